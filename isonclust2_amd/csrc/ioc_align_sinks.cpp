// ioc_align_sinks.cpp — the entry points of the batched GPU aligner that ask for the alignment itself, and the consensus call on
// top of them: each describes where the walks' operation bytes go (AlnSink, ioc_align_sink.h) and runs ioc_align_pairs_sink
// (ioc_align_gpu.hip).  Host code only: the kernels are behind the iock_* launchers.  An entry point checks its arguments, plans its
// segments and pairs on the host (SinkPlan, ioc_sink_plan.h) and runs device stages in a row (SinkRun): pile -> sites -> alleles ->
// [split] -> [group pile -> call] -> copy-out for the alleles family, pile -> call -> copy-out for the polish family, pile -> correct ->
// copy-out for the read correction, pile -> blocks -> [inserts -> [windows | variants] -> [full]] | [ends] | [polish] | [correct] -> copy-out for the
// block family (ten entry points, one record and one runner: BlocksCall, align_pairs_blocks_call), upload -> the same stage for the
// calls that bring their own tables.  A stage takes device pointers and says where it left what it made; none calls the next.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <functional>
#include <optional>
#include <string>
#include <vector>

#include "ioc_align_sink.h"
#include "ioc_group_pile.h"
#include "ioc_group_pile_weighted.h"
#include "ioc_internal.h"
#include "ioc_plane_pile.h"
#include "ioc_read_blocks.h"
#include "ioc_read_correct.h"
#include "ioc_iso_correct.h"
#include "ioc_read_inserts.h"
#include "ioc_read_ends.h"
#include "ioc_insert_windows.h"
#include "ioc_window_variants.h"
#include "ioc_iso_splice.h"

namespace {
struct AlnCall {  // what every aligning entry point passes on
    int32_t n_pairs;
    const ioc_aln_pair* pairs;
    int32_t k, match, mismatch, gap_extend;
    int32_t* score;
    int64_t* windows;
    double* ratio;
    int run(ioc_ctx* c, const AlnSink* sink) const { return ioc_align_pairs_sink(c, n_pairs, pairs, k, match, mismatch, gap_extend, score, windows, ratio, sink); }
};

struct SitesRule {  // the thresholds of a site search, and those ioc_host_pileup_sites refuses
    int32_t min_depth, min_alt, min_pct, max_sites;
    bool ok() const { return min_depth >= 1 && min_alt >= 1 && min_pct >= 1 && min_pct <= 50 && max_sites >= 1; }
};
struct SplitCall {  // what a split is run with and where it leaves what it made (ioc_host_alleles_split's parameters and outputs, per call)
    int32_t min_link, min_margin, rounds;
    int64_t* out_link;
    int8_t* out_phase;
    uint8_t* out_group;
    int32_t* out_vote;
    ioc_split_seg* out_seg;
    bool ok() const { return min_link >= 1 && min_margin >= 1 && rounds >= 0 && rounds <= 64; }  // (what ioc_host_alleles_split refuses)
};
struct CallOut {  // the least depth a consensus call calls at and where it leaves what it called (cap: what seq and qual hold each)
    int32_t min_depth;
    char *seq, *qual;
    int64_t cap;
    int64_t* off;
    ioc_polish_stats* stats;
    bool ok() const { return min_depth >= 1 && off && cap >= 0; }
};
struct GroupPolish {  // the call of both groups of every segment of a split, and where their tables go (ioc_planes_polish's outputs)
    CallOut call;
    ioc_pileup_col* out_gcols;
    ioc_pileup_ins* out_gins;
};
struct CorrectOut {  // the rule of a read correction and where it leaves every pair's bytes (cap: what seq and qual hold each)
    ReadRule rule;
    char *seq, *qual;
    int64_t cap;
    int64_t* off;
    ioc_correct_stats* stats;
    bool ok() const { return rule.ok() && off && cap >= 0; }
};
struct IsoCorrectOut {  // the rule of a read correction by isoform and where it leaves every pair's bytes (cap: what seq and qual hold each)
    ReadRule rule;
    char *seq, *qual;
    int64_t cap;
    int64_t* off;
    ioc_iso_correct_stats* stats;
    bool ok() const { return rule.ok() && off && cap >= 0; }
};
struct BlocksOut {  // the rule of a block search and where it leaves what it made (cap: the records `blocks` holds)
    BlocksRule rule;
    ioc_block_row* rows;
    ioc_pile_block* blocks;
    int64_t cap;
    int64_t* block_off;
    ioc_read_blocks* reads;
    ioc_blocks_seg* seg;
    bool ok() const { return rule.ok() && block_off && cap >= 0; }
};
struct InsertsOut {  // the rule of a search for insertion sites and where it leaves what it made (cap: the records `sites` holds)
    InsertsRule rule;
    ioc_insert_row* rows;
    ioc_pile_insert* sites;
    int64_t cap;
    int64_t* site_off;
    ioc_read_inserts* reads;
    ioc_inserts_seg* seg;
    bool ok() const { return rule.ok() && site_off && cap >= 0; }
};
struct EndsOut {  // the rule of a search for ends and where it leaves what it made (cap / vcap: the records `sites` / `variants` hold)
    EndsRule rule;
    ioc_end_row* rows;
    ioc_end_site* sites;
    int64_t cap;
    int64_t* site_off;
    ioc_end_variant* variants;
    int64_t vcap;
    int64_t* var_off;
    ioc_read_ends* reads;
    ioc_ends_seg* seg;
    bool ok() const { return rule.ok() && site_off && var_off && cap >= 0 && vcap >= 0; }
};
// the block stage's words an insert search combines with its own: the host's (uploaded), the device's (where the block stage left
// them), or none (all NULL); pre_full is the host's, a word per segment
struct InsertsPre {
    const uint64_t *host_key = nullptr, *host_mask = nullptr, *pre_full = nullptr;
    const unsigned long long *dev_key = nullptr, *dev_mask = nullptr;
    uint32_t dev_key_stride = 1, dev_mask_stride = 1;
};
// what a call refuses once its bound is known: IOC_OK, or the status with the message set
int call_room_ok(ioc_ctx* c, const std::string& who, const CallOut& o, int64_t bound)
{
    if (o.cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": cap " + std::to_string(o.cap) + " below the bound " + std::to_string(bound));
    return bound > 0 && (!o.seq || !o.qual) ? IOC_ERR_ARG : IOC_OK;
}

// what a pile that projects (`plane` given) lays down beside the base and the ins planes: the six slot planes, the seven weight
// planes (which ask for the slot planes and for the pool's qualities), the length plane, the position plane
struct PileProject {
    bool ins = false, weights = false, ilen = false, qpos = false;
};

// ---- where the stages leave what they made (device pointers) ----
struct PiledDev {  // pile: the tables of the kind (a_pile; a_pile_ins or a_pile_w) and, where it projects, the planes (a_planes)
    ioc_pileup_col *cols, *wcols;
    ioc_pileup_ins *ins, *wins;
    uint8_t *base, *insf, *slots, *weights;
    uint8_t* ilen = nullptr;  // (a pile that projects the length plane: behind every other plane)
    uint32_t* qpos = nullptr;  // (a pile that projects the position plane: behind the length plane, at a multiple of 16 bytes)
};
struct BlocksDev {  // blocks (a_blocks): where the block stage left every pair's record (its key) and its mask
    const ioc_read_blocks* reads;
    const unsigned long long* mask;
};
struct SitesDev {  // sites (a_call): the segments, what was kept, and the room of the allele gather behind them
    const IocPileSeg* segs;
    const ioc_pile_site* sites;
    const int64_t* site_off;
    int32_t* seg_of_pair;
    uint64_t* plane;
    int64_t* allele_off;
    uint8_t* alleles;
};
struct GroupPiled {  // group pile (a_gpile): the tables of the 2 n group-segments, twice the plan's rows, and the group-segments themselves (the host's)
    std::vector<IocPileSeg> gsegs;
    ioc_pileup_col* cols;
    ioc_pileup_ins* ins;
    ioc_pileup_col* wcols = nullptr;  // (groups_pile, weighted: cols holds the counts, these the sums of weights; ins is not made)
    ioc_pileup_ins* wins = nullptr;
    int64_t n_rows = 0;  // (groups_pile: the rows of its tables, the sum over the group-segments of rlen + 1, ...
    GroupMemberLists lists;           // ... every group's member list and ...
    std::vector<IocGroupWork> work;   // ... the work items, which the uploads read until the call stage has waited for the stream)
    const IocPileSeg* dev_gsegs = nullptr;            // (groups_pile: the group-segments on the device, and the base and the slot planes it
    const uint8_t *base = nullptr, *slots = nullptr;  // piled from, where they lay or where it uploaded them: all in a_gpile or the caller's)
};
struct IsoPolish {  // the call of the first min(n_groups, max_iso) isoforms of every segment behind a block search (ioc_align_pairs_blocks_polish)
    int32_t max_iso;
    CallOut call;
    int64_t iso_cap;
    int64_t* iso_off;
    bool weighted = false;  // (ioc_align_pairs_blocks_polish_weighted: every isoform called by weight)
    bool ok() const { return max_iso >= 1 && call.ok() && iso_cap >= 0 && iso_off; }
};
// split (a_split): the member lists and the group bytes.  What a group pile reads beside the plan: those and the planes, on the
// device (a NULL pointer: the array is the host's — Planes::host — and uploaded; ioc_planes_polish: all of them, behind a split: none)
struct Planes {
    const uint32_t *mem_off, *members;
    const uint8_t *group, *base, *slots;
    // (a weighted groups pile) the seven weight planes: on the device one behind the other, [wbase plane][wslot planes x 6]; the
    // host's as the caller holds them, wbase and wslots
    const uint8_t *weights = nullptr, *wbase = nullptr, *wslots = nullptr;
};
// the length and the position plane beside those (the read correction by isoform): the host's, or the device's where a pile projected them
struct LongPlanes {
    const uint8_t* ilen = nullptr;
    const uint32_t* qpos = nullptr;
};
struct Out { void* dst; const void* src; size_t bytes; };  // a block that goes back to the host where the caller asked for it (dst NULL: not)

// The events that time every kernel of a stage on its own under IOC_TRACE: one in front of each of the `kernels` and one behind the
// last, or none.  events() is what the stage's launcher takes (NULL: none); once the stream has been waited for, add_to(ms) adds
// what lay between every two to ms[0 .. kernels).
struct KernelTimes {
    EventSet each;
    int create(ioc_ctx* c, size_t kernels)
    {
        if (!getenv("IOC_TRACE")) return IOC_OK;
        each.v.assign(kernels + 1, nullptr);
        for (auto& e : each.v) IOC_CHK(c, hipEventCreate(&e));
        return IOC_OK;
    }
    bool on() const { return !each.v.empty(); }
    hipEvent_t* events() { return on() ? each.v.data() : nullptr; }
    void add_to(double* ms) const
    {
        for (size_t x = 0; x + 1 < each.v.size(); ++x) {
            float one = 0;
            if (hipEventElapsedTime(&one, each.v[x], each.v[x + 1]) == hipSuccess) ms[x] += double(one);
        }
    }
};

// One call's stages over a context, the tally of its trace line and the device time of its launches: begin / end record an event
// either side of a launch (timed false: none is created), and settled(), once the stream has been waited for, adds what lay
// between them to `ms`.
struct SinkRun {
    struct Timed { hipEvent_t a, b; double* into; };
    ioc_ctx* c;
    AlnTally t;
    std::vector<Timed> ev;  // (destroyed on every way out, the IOC_CHK returns included)
    size_t done = 0;
    bool timing = true;
    ~SinkRun() { for (Timed& e : ev) (void)(e.a && hipEventDestroy(e.a)), (void)(e.b && hipEventDestroy(e.b)); }
    int begin(double& ms, bool timed = true)
    {
        if (!(timing = timed)) return IOC_OK;
        ev.push_back(Timed{nullptr, nullptr, &ms});
        IOC_CHK(c, hipEventCreate(&ev.back().a));
        IOC_CHK(c, hipEventCreate(&ev.back().b));
        IOC_CHK(c, hipEventRecord(ev.back().a, c->stream));
        return IOC_OK;
    }
    int end() { if (timing) IOC_CHK(c, hipEventRecord(ev.back().b, c->stream)); return IOC_OK; }
    void settled()
    {
        for (float ms = 0; done < ev.size(); ++done)
            if (hipEventElapsedTime(&ms, ev[done].a, ev[done].b) == hipSuccess) *ev[done].into += double(ms);
    }
    // the blocks that are asked for, copied from the device: the host's time over it to t.ms_copy, the bytes to t.copied
    int copy_out(std::initializer_list<Out> outs)
    {
        const auto t0 = std::chrono::steady_clock::now();
        for (const Out& o : outs)
            if (o.dst && o.bytes) {
                IOC_CHK(c, hipMemcpy(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost));
                t.copied += int64_t(o.bytes);
            }
        t.ms_copy += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return IOC_OK;
    }
    int pile(const AlnCall& a, PileKind kind, ioc_aln_stats* out_stats, const int64_t* row_base, int64_t n_rows, const int64_t* plane, int64_t plane_bytes, PileProject project,
             PiledDev& d);
    int sites(const SitesRule& r, const SinkPlan& p, const ioc_pileup_col* d_cols, ioc_pile_site* out_sites, int64_t* site_off, int64_t* n_found, SitesDev& d);
    int alleles(const SitesDev& d, const SinkPlan& p, const int32_t* seg_of_pair, const PiledDev& planes, const int64_t* site_off, int64_t* allele_off, uint8_t* out_alleles);
    int split(const SplitCall& sp, size_t n, size_t np, const int32_t* seg_of_pair, const int64_t* site_off, const int64_t* allele_off, const ioc_pile_site* sites,
              const uint8_t* alleles, bool on_device, Planes& d);
    int group_pile(const SinkPlan& p, const int32_t* seg_of_pair, const Planes& host, Planes dev, GroupPiled& d);
    int groups_pile(const SinkPlan& p, const int32_t* seg_of_pair, const int32_t* group, const int32_t* n_groups, const Planes& host, Planes dev, GroupPiled& d,
                    bool weighted = false, int32_t all_below = 0);
    int iso_correct(const SinkPlan& p, const int32_t* seg_of_pair, const int32_t* group, const int32_t* n_groups, const uint8_t* d_frames, uint64_t frame_bytes,
                    const Planes& host, Planes dev, const LongPlanes& host_long, LongPlanes dev_long, const std::vector<uint64_t>& q_off, const std::vector<uint32_t>& q_len,
                    const IsoCorrectOut& o);
    int correct(const SinkPlan& p, const int32_t* seg_of_pair, const uint8_t* d_frames, uint64_t frame_bytes, const ioc_pileup_col* d_cols, const ioc_pileup_ins* d_ins,
                const Planes& host, Planes dev, const CorrectOut& o);
    int blocks(const SinkPlan& p, const int32_t* seg_of_pair, const uint8_t* host_base, const uint8_t* dev_base, const BlocksOut& o, BlocksDev* where = nullptr);
    int inserts(const SinkPlan& p, const int32_t* seg_of_pair, const uint8_t* host_base, const uint8_t* host_ilen, const uint8_t* dev_base, const uint8_t* dev_ilen,
                const InsertsPre& pre, const InsertsOut& o);
    int ends(const SinkPlan& p, const int32_t* seg_of_pair, const ioc_read_extent* extents, const int32_t* host_pre, const int32_t* dev_pre, uint32_t dev_pre_stride,
             const EndsOut& o);
};

// Pile and project.  The tables of `kind`, n_rows records each — a_pile; a_pile_ins beside it (ins), or a_pile_w as [wcols][wins] (weighted)
// — are reserved and zeroed and the pairs aligned into them (k_ops_pileup adds, where the walks' bytes lie, slice after slice and re-run after
// re-run).  `plane` (the alleles family): every pair is projected as well, into the planes of a_planes, [base planes][ins planes] and, with
// pj.ins, [slot planes x 6] behind them, set to IOC_ALLELE_NONE / 0 once here; with pj.weights (which asks for pj.ins
// and for the pool's qualities), [weight planes x 7] behind those, set to 0 with them.  A call without pj.weights reserves what
// it always did.  pj.ilen: one more plane behind all of those, the length plane (k_ops_project_ilen), set to 0 with them.
// pj.qpos: behind that, from the next multiple of 16 bytes on, the position plane (k_ops_project_qpos), four bytes a row, set to 0.
int SinkRun::pile(const AlnCall& a, PileKind kind, ioc_aln_stats* out_stats, const int64_t* row_base, int64_t n_rows, const int64_t* plane,
                  int64_t plane_bytes, PileProject pj, PiledDev& d)
{
    IOC_CHK(c, hipSetDevice(c->device));
    const size_t b_cols = size_t(n_rows) * sizeof(ioc_pileup_col), b_ins = size_t(n_rows) * sizeof(ioc_pileup_ins);
    std::vector<int64_t> len(size_t(a.n_pairs), 0);
    std::vector<uint8_t> piled(size_t(a.n_pairs), 0);
    const bool weighted = kind == PileKind::weighted;
    DevBuf* second = kind == PileKind::ins ? &c->a_pile_ins : weighted ? &c->a_pile_w : nullptr;  // [ins], or [wcols][wins]
    const size_t b_second = weighted ? b_cols + b_ins : b_ins;
    IOC_TRY(ioc_reserve(c, c->a_pile, b_cols));
    if (second) IOC_TRY(ioc_reserve(c, *second, b_second));
    IOC_CHK(c, hipMemsetAsync(c->a_pile.p, 0, b_cols, c->stream));
    if (second) IOC_CHK(c, hipMemsetAsync(second->p, 0, b_second, c->stream));
    AlnSink::Pile pl{kind, c->a_pile.as<ioc_pileup_col>(), nullptr, nullptr, nullptr, n_rows, row_base, piled.data()};
    if (kind == PileKind::ins) pl.ins = second->as<ioc_pileup_ins>();
    if (weighted) pl.wcols = second->as<ioc_pileup_col>(), pl.wins = reinterpret_cast<ioc_pileup_ins*>(second->as<uint8_t>() + b_cols);  // (b_cols: a multiple of 32)
    if (plane) {
        const size_t b_plane = size_t(plane_bytes);
        const size_t n_zeroed = !pj.ins ? 1 : 1 + size_t(IOC_PILE_INS_SLOTS) + (pj.weights ? size_t(IOC_WEIGHT_PLANES) : 0);  // (the ins planes and on)
        const size_t b_bytes = (1 + n_zeroed + (pj.ilen ? 1 : 0)) * b_plane, o_qpos = (b_bytes + 15) & ~size_t(15);
        IOC_TRY(ioc_reserve(c, c->a_planes, pj.qpos ? o_qpos + 4 * b_plane : b_bytes));
        pl.project = true, pl.base_planes = c->a_planes.as<uint8_t>(), pl.ins_planes = pl.base_planes + b_plane;
        pl.plane_bytes = plane_bytes, pl.plane = plane;
        if (pj.ins) pl.project_ins = true, pl.slot_planes = pl.base_planes + 2 * b_plane;
        if (pj.ins && pj.weights) pl.project_weights = true, pl.weight_planes = pl.slot_planes + size_t(IOC_PILE_INS_SLOTS) * b_plane;
        if (pj.ilen) pl.project_ilen = true, pl.ilen_planes = pl.base_planes + (1 + n_zeroed) * b_plane;
        if (pj.qpos) pl.project_qpos = true, pl.qpos_planes = reinterpret_cast<uint32_t*>(pl.base_planes + o_qpos);
        if (b_plane > 0) {
            IOC_CHK(c, hipMemsetAsync(pl.base_planes, IOC_ALLELE_NONE, b_plane, c->stream));
            IOC_CHK(c, hipMemsetAsync(pl.ins_planes, 0, (n_zeroed + (pj.ilen ? 1 : 0)) * b_plane, c->stream));  // (and the slot, weight and length planes)
            if (pj.qpos) IOC_CHK(c, hipMemsetAsync(pl.qpos_planes, 0, 4 * b_plane, c->stream));
        }
    }
    const AlnSink sink{SinkKind::reduced, len.data(), &t, {}, out_stats != nullptr, out_stats, pl};
    IOC_TRY(a.run(c, a.n_pairs > 0 ? &sink : nullptr));
    d = PiledDev{pl.cols, pl.wcols, pl.ins, pl.wins, pl.base_planes, pl.ins_planes, pl.slot_planes, pl.weight_planes, pl.ilen_planes, pl.qpos_planes};
    return IOC_OK;
}

// The site search over a table that lies on the device, and the sites copied back: a_call holds [segments][seg_len][site_off]
// [n_found][sites] and behind them the allele gather's [seg_of_pair][plane][allele_off][alleles].
int SinkRun::sites(const SitesRule& r, const SinkPlan& pn, const ioc_pileup_col* d_cols, ioc_pile_site* out_sites, int64_t* site_off, int64_t* n_found, SitesDev& d)
{
    const size_t n = pn.segs.size(), np = pn.plane.size(), bound = size_t(pile_sites_bound(pn.segs, r.max_sites));
    Arena l;
    const size_t o_seg = l.take(n * sizeof(IocPileSeg)), o_len = l.take(n * 8), o_off = l.take((n + 1) * 8), o_found = l.take(n * 8),
                 o_sites = l.take(bound * sizeof(ioc_pile_site)), o_sop = l.take(np * 4), o_plane = l.take(np * 8), o_aoff = l.take((np + 1) * 8),
                 o_all = l.take(size_t(pn.alleles_bound));
    IOC_TRY(ioc_reserve(c, c->a_call, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_call.p);
    d = SitesDev{reinterpret_cast<const IocPileSeg*>(p + o_seg), reinterpret_cast<const ioc_pile_site*>(p + o_sites), reinterpret_cast<const int64_t*>(p + o_off),
                 reinterpret_cast<int32_t*>(p + o_sop), reinterpret_cast<uint64_t*>(p + o_plane), reinterpret_cast<int64_t*>(p + o_aoff), p + o_all};
    IOC_CHK(c, hipMemcpyAsync(p + o_seg, pn.segs.data(), n * sizeof(IocPileSeg), hipMemcpyHostToDevice, c->stream));
    IOC_TRY(begin(t.ms_sites));
    IOC_CHK(c, iock_pile_sites(c->stream, d.segs, uint32_t(n), d_cols, uint64_t(pn.n_rows), r.min_depth, r.min_alt, r.min_pct, r.max_sites,
                               reinterpret_cast<int64_t*>(p + o_found), reinterpret_cast<int64_t*>(p + o_len), reinterpret_cast<int64_t*>(p + o_off),
                               reinterpret_cast<ioc_pile_site*>(p + o_sites), uint64_t(bound)));
    IOC_TRY(end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    settled();
    IOC_TRY(copy_out({{site_off, p + o_off, (n + 1) * 8}, {n_found, p + o_found, n * 8}}));
    const int64_t kept = site_off[n];
    if (kept < 0 || size_t(kept) > bound) return ioc_fail(c, IOC_ERR_HIP, "the site search returned a count outside its bound");
    return copy_out({{out_sites, d.sites, size_t(kept) * sizeof(ioc_pile_site)}});
}

// k_site_alleles over the planes where the pile left them and the sites where the search did, and the alleles copied back where
// they are asked for: one byte per (pair, kept site of its segment), pair i's from allele_off[i] on.
int SinkRun::alleles(const SitesDev& d, const SinkPlan& pn, const int32_t* seg_of_pair, const PiledDev& planes, const int64_t* site_off, int64_t* allele_off,
                     uint8_t* out_alleles)
{
    const size_t n = pn.segs.size(), np = pn.plane.size();
    allele_off[0] = 0;
    for (size_t i = 0; i < np; ++i) allele_off[i + 1] = allele_off[i] + (site_off[seg_of_pair[i] + 1] - site_off[seg_of_pair[i]]);
    const int64_t bytes = allele_off[np];
    if (bytes > pn.alleles_bound) return ioc_fail(c, IOC_ERR_HIP, "the site search kept more sites than its bound");
    if (bytes == 0) return IOC_OK;
    IOC_CHK(c, hipMemcpyAsync(d.seg_of_pair, seg_of_pair, np * 4, hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemcpyAsync(d.plane, pn.plane.data(), np * 8, hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemcpyAsync(d.allele_off, allele_off, (np + 1) * 8, hipMemcpyHostToDevice, c->stream));
    IOC_TRY(begin(t.ms_alleles));
    IOC_CHK(c, iock_site_alleles(c->stream, uint32_t(np), d.seg_of_pair, d.segs, uint32_t(n), d.plane, planes.base, planes.insf, uint64_t(pn.plane_bytes), d.sites,
                                 d.site_off, d.allele_off, d.alleles, uint64_t(bytes)));
    IOC_TRY(end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    settled();
    return copy_out({{out_alleles, d.alleles, size_t(bytes)}});
}

// The split kernels (ioc_site_split.hip) over sites and alleles that lie on the device — or on the host (on_device false), and are
// uploaded then — and what they made copied back.  site_off / allele_off / seg_of_pair are the host's.  a_split holds, in this
// order, the host's tables [site_off][allele_off][seg_of_pair][mem_off][members][word_off][bit_off][tile_seg][seg_of_site], the
// kernels' own [marks][bits minor][bits major][g1][g0][link][phase][seed][group][vote][records] and, uploaded, [sites][alleles].
// Under IOC_TRACE the steps are timed one by one (t.ms_split, in the order of IocSplitStep).
int SinkRun::split(const SplitCall& sp, size_t n, size_t np, const int32_t* seg_of_pair, const int64_t* site_off, const int64_t* allele_off,
                   const ioc_pile_site* sites, const uint8_t* alleles, bool on_device, Planes& d)
{
    const MemberLists m = member_lists(n, np, seg_of_pair);
    const SplitTables s = split_tables(n, site_off, m.mem_off);
    const size_t S = n ? size_t(site_off[n]) : 0, bytes = np ? size_t(allele_off[np]) : 0, T = s.T, P = s.P;
    Arena l;
    const size_t o_soff = l.take((n + 1) * 8), o_aoff = l.take((np + 1) * 8), o_sop = l.take(np * 4), o_moff = l.take((n + 1) * 4), o_mem = l.take(np * 4),
                 o_woff = l.take((n + 1) * 4), o_boff = l.take((n + 1) * 8), o_tseg = l.take(T * 4), o_sos = l.take(S * 4), tables = l.size();
    const size_t o_marks = l.take(S * 8), o_bm = l.take(P * 8), o_bM = l.take(P * 8), o_g1 = l.take(T * 8), o_g0 = l.take(T * 8), o_link = l.take(S * 8),
                 o_phase = l.take(S), o_seed = l.take(n * 4), o_group = l.take(np), o_vote = l.take(np * 4), o_rec = l.take(n * sizeof(ioc_split_seg));
    const size_t o_sites = l.take(on_device ? 0 : S * sizeof(ioc_pile_site)), o_all = l.take(on_device ? 0 : bytes);
    std::vector<uint8_t> stage(tables, 0);
    const int64_t zero = 0;
    auto put = [&](size_t o, const void* src, size_t b) { if (b) memcpy(stage.data() + o, src, b); };
    put(o_soff, n ? site_off : &zero, (n + 1) * 8), put(o_aoff, np ? allele_off : &zero, (np + 1) * 8), put(o_sop, seg_of_pair, np * 4);
    put(o_moff, m.mem_off.data(), (n + 1) * 4), put(o_mem, m.members.data(), np * 4), put(o_woff, s.word_off.data(), (n + 1) * 4);
    put(o_boff, s.bit_off.data(), (n + 1) * 8), put(o_tseg, s.tile_seg.data(), T * 4), put(o_sos, s.seg_of_site.data(), S * 4);
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_split, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_split.p);
    IOC_CHK(c, hipMemcpyAsync(p, stage.data(), tables, hipMemcpyHostToDevice, c->stream));
    t.split_uploaded += int64_t(tables);
    if (!on_device) {
        if (S) IOC_CHK(c, hipMemcpyAsync(p + o_sites, sites, S * sizeof(ioc_pile_site), hipMemcpyHostToDevice, c->stream));
        if (bytes) IOC_CHK(c, hipMemcpyAsync(p + o_all, alleles, bytes, hipMemcpyHostToDevice, c->stream));
        t.split_uploaded += int64_t(S * sizeof(ioc_pile_site) + bytes);
    }
    auto u64p = [&](size_t o) { return reinterpret_cast<unsigned long long*>(p + o); };
    d.mem_off = reinterpret_cast<const uint32_t*>(p + o_moff), d.members = reinterpret_cast<const uint32_t*>(p + o_mem), d.group = p + o_group;
    const IocSplitDev v{uint32_t(n), uint32_t(np), uint32_t(T), uint64_t(S), uint64_t(bytes), uint64_t(P), uint64_t(s.most),
                        on_device ? sites : reinterpret_cast<const ioc_pile_site*>(p + o_sites), reinterpret_cast<const long long*>(p + o_soff),
                        on_device ? alleles : p + o_all, reinterpret_cast<const long long*>(p + o_aoff), reinterpret_cast<const int32_t*>(p + o_sop),
                        d.mem_off, d.members, reinterpret_cast<const uint32_t*>(p + o_woff), reinterpret_cast<const long long*>(p + o_boff),
                        reinterpret_cast<const int32_t*>(p + o_tseg), reinterpret_cast<const int32_t*>(p + o_sos), reinterpret_cast<int2*>(p + o_marks),
                        u64p(o_bm), u64p(o_bM), u64p(o_g1), u64p(o_g0), reinterpret_cast<long long*>(p + o_link), reinterpret_cast<int8_t*>(p + o_phase),
                        reinterpret_cast<int32_t*>(p + o_seed), p + o_group, reinterpret_cast<int32_t*>(p + o_vote), reinterpret_cast<ioc_split_seg*>(p + o_rec)};
    std::vector<IocSplitStep> steps{IocSplitStep::marks, IocSplitStep::bits, IocSplitStep::link, IocSplitStep::seed, IocSplitStep::phase0, IocSplitStep::vote};
    for (int32_t r = 0; r < sp.rounds; ++r) steps.insert(steps.end(), {IocSplitStep::group_bits, IocSplitStep::rephase, IocSplitStep::vote});
    steps.push_back(IocSplitStep::record);
    const bool timed = getenv("IOC_TRACE") != nullptr;
    for (IocSplitStep step : steps) {
        IOC_TRY(begin(t.ms_split[size_t(step)], timed));
        IOC_CHK(c, iock_site_split(c->stream, v, step, sp.min_link, sp.min_margin));
        IOC_TRY(end());
    }
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    settled();
    return copy_out({{sp.out_link, p + o_link, S * 8}, {sp.out_phase, p + o_phase, S}, {sp.out_group, p + o_group, np}, {sp.out_vote, p + o_vote, np * 4},
                     {sp.out_seg, p + o_rec, n * sizeof(ioc_split_seg)}});
}

// the split's part of a trace line
std::string split_trace(const AlnTally& t)
{
    char buf[480];
    snprintf(buf, sizeof buf, "k_site_marks %.3f ms, k_allele_bits %.3f ms, k_site_link %.3f ms, k_split_seed %.3f ms, k_split_phase0 %.3f ms, k_split_vote %.3f ms, k_group_bits %.3f ms, k_split_rephase %.3f ms, k_split_record %.3f ms, %lld bytes uploaded",
             t.ms_split[0], t.ms_split[1], t.ms_split[2], t.ms_split[3], t.ms_split[4], t.ms_split[5], t.ms_split[6], t.ms_split[7], t.ms_split[8],
             (long long)t.split_uploaded);
    return buf;
}

// k_plane_pile over the 2 n group-segments of the plan's segments: a_gpile holds [group-segments][work items][plane offsets][mem_off]
// [members][group][base plane][slot planes][gcols][gins], the middle five only where they are uploaded.  Group-segment 2 g + h
// owns the rows 2 * row0(g) + h * (rlen(g) + 1) .. of both tables, which are set to 0 first: k_plane_pile is launched over the
// group-segments that have reads alone.  The stream is not waited for: the call stage behind it does that.
int SinkRun::group_pile(const SinkPlan& pn, const int32_t* seg_of_pair, const Planes& ph, Planes pd, GroupPiled& d)
{
    const std::vector<IocPileSeg>& ds = pn.segs;
    const size_t n = ds.size(), np = pn.plane.size(), P = size_t(pn.plane_bytes);
    const int64_t n_rows = 2 * pn.n_rows;
    std::vector<IocPileSeg>& gsegs = d.gsegs = std::vector<IocPileSeg>(2 * n);
    std::vector<uint32_t> reads(2 * n, 0);
    for (size_t g = 0; g < n; ++g)
        for (int64_t h = 0; h < 2; ++h) gsegs[2 * g + size_t(h)] = IocPileSeg{2 * ds[g].row0 + h * (int64_t(ds[g].rlen) + 1), ds[g].f_off, ds[g].rlen, ds[g].rc};
    for (size_t i = 0; i < np; ++i)
        if (ph.group[i] <= 1) ++reads[2 * size_t(seg_of_pair[i]) + ph.group[i]];
    std::vector<IocPlaneWork> work;
    for (size_t x = 0; x < 2 * n; ++x)
        for (int64_t row = 0; reads[x] > 0 && row <= int64_t(gsegs[x].rlen); row += IOC_PLANE_PILE_ROWS) work.push_back(IocPlaneWork{uint32_t(x), uint32_t(row)});
    if (work.size() > size_t(INT32_MAX)) return ioc_fail(c, IOC_ERR_CAPACITY, "the group tables have more than 2^31 - 1 blocks of rows");
    const MemberLists m = pd.members ? MemberLists{} : member_lists(n, np, seg_of_pair);  // (as the split has them)
    Arena l;
    const size_t o_gseg = l.take(2 * n * sizeof(IocPileSeg)), o_work = l.take(work.size() * sizeof(IocPlaneWork)), o_plane = l.take(np * 8),
                 o_moff = l.take(pd.members ? 0 : (n + 1) * 4), o_mem = l.take(pd.members ? 0 : np * 4), o_group = l.take(pd.group ? 0 : np),
                 o_base = l.take(pd.base ? 0 : P), o_slots = l.take(pd.slots ? 0 : size_t(IOC_PILE_INS_SLOTS) * P),
                 o_cols = l.take(size_t(n_rows) * sizeof(ioc_pileup_col)), o_ins = l.take(size_t(n_rows) * sizeof(ioc_pileup_ins));
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_gpile, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_gpile.p);
    auto up = [&](size_t o, const void* src, size_t b) { return b ? hipMemcpyAsync(p + o, src, b, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
    IOC_CHK(c, up(o_gseg, gsegs.data(), 2 * n * sizeof(IocPileSeg)));
    IOC_CHK(c, up(o_work, work.data(), work.size() * sizeof(IocPlaneWork)));
    IOC_CHK(c, up(o_plane, pn.plane.data(), np * 8));
    auto place = [&](auto& dev, size_t o, const void* src, size_t b) {  // (what does not lie on the device yet is uploaded)
        return dev ? hipSuccess : (dev = reinterpret_cast<decltype(+dev)>(p + o), up(o, src, b));
    };
    IOC_CHK(c, place(pd.mem_off, o_moff, m.mem_off.data(), (n + 1) * 4));
    IOC_CHK(c, place(pd.members, o_mem, m.members.data(), np * 4));
    IOC_CHK(c, place(pd.group, o_group, ph.group, np));
    IOC_CHK(c, place(pd.base, o_base, ph.base, P));
    IOC_CHK(c, place(pd.slots, o_slots, ph.slots, size_t(IOC_PILE_INS_SLOTS) * P));
    d.cols = reinterpret_cast<ioc_pileup_col*>(p + o_cols), d.ins = reinterpret_cast<ioc_pileup_ins*>(p + o_ins);
    if (n_rows > 0) IOC_CHK(c, hipMemsetAsync(p + o_cols, 0, l.size() - o_cols, c->stream));
    IOC_TRY(begin(t.ms_plane_pile));
    IOC_CHK(c, iock_plane_pile(c->stream, reinterpret_cast<const IocPlaneWork*>(p + o_work), uint32_t(work.size()), reinterpret_cast<const IocPileSeg*>(p + o_gseg),
                               pd.mem_off, pd.members, uint32_t(np), pd.group, reinterpret_cast<const uint64_t*>(p + o_plane), pd.base, pd.slots,
                               uint64_t(P), d.cols, d.ins, uint64_t(n_rows)));
    return end();
}

// k_group_pile over the G group-segments of the plan's segments, n_groups[g] of segment g in segment order: a_gpile holds
// [group-segments][work items][plane offsets][gmem_off][gmembers][base plane][slot planes][gcols][gins], the planes only where they
// are uploaded.  Every group's own member list is made on the host (group_member_lists) and uploaded, 4 bytes a pair that is in a
// group.  Group-segment x owns the rows of both tables from the sum over the earlier group-segments of (rlen + 1) on; the tables
// are set to 0 first: k_group_pile is launched over the group-segments that have reads alone.  The stream is not waited for: the
// call stage behind it does that.  G is at least 1.  weighted: k_group_pile_weighted in its place, over the seven weight planes
// as well ([weight planes] behind the slot planes where they are uploaded), and the tables are [gcols][gwcols][gwins].
// all_below > 0 (the read correction by isoform, its min_depth): behind the group-segments stands one more per segment that lists
// all of its pairs, whatever their group — group-segment gseg_off[n] + g, n more in all, piled by the same launch.  A segment whose
// pairs are all in groups of at least all_below members holds nobody against that table (iso_uses_group): its list stays empty
// and nothing is piled for it.
int SinkRun::groups_pile(const SinkPlan& pn, const int32_t* seg_of_pair, const int32_t* group, const int32_t* n_groups, const Planes& ph, Planes pd, GroupPiled& d,
                         bool weighted, int32_t all_below)
{
    const bool with_all = all_below > 0;
    const std::vector<IocPileSeg>& ds = pn.segs;
    const size_t n = ds.size(), np = pn.plane.size(), P = size_t(pn.plane_bytes);
    GroupMemberLists& m = d.lists = group_member_lists(n, np, seg_of_pair, group, n_groups);
    const size_t G = m.gseg_off[n] + (with_all ? n : 0);
    std::vector<IocPileSeg>& gsegs = d.gsegs = std::vector<IocPileSeg>(G);
    d.n_rows = 0;
    for (size_t g = 0; g < n; ++g)
        for (size_t x = m.gseg_off[g]; x < m.gseg_off[g + 1]; ++x) {
            gsegs[x] = IocPileSeg{d.n_rows, ds[g].f_off, ds[g].rlen, ds[g].rc};
            d.n_rows += int64_t(ds[g].rlen) + 1;
        }
    if (with_all) {
        const MemberLists all = member_lists(n, np, seg_of_pair);
        std::vector<uint8_t> needed(n, 0);  // some pair of the segment is in no group, or in one of fewer than all_below members
        for (size_t i = 0; i < np; ++i) {
            const size_t g = size_t(seg_of_pair[i]);
            const bool in_group = group[i] >= 0 && group[i] < n_groups[g];
            const size_t x = in_group ? m.gseg_off[g] + size_t(group[i]) : 0;
            if (!in_group || !iso_uses_group(group[i], m.gmem_off[x + 1] - m.gmem_off[x], all_below)) needed[g] = 1;
        }
        std::vector<uint32_t> off(m.gmem_off), mem(m.gmembers);
        off.reserve(G + 1), mem.reserve(m.gmembers.size() + np);
        for (size_t g = 0; g < n; ++g) {
            for (uint32_t y = all.mem_off[g]; needed[g] && y < all.mem_off[g + 1]; ++y) mem.emplace_back(all.members[y]);
            off.emplace_back(uint32_t(mem.size()));
            gsegs[m.gseg_off[n] + g] = IocPileSeg{d.n_rows, ds[g].f_off, ds[g].rlen, ds[g].rc};
            d.n_rows += int64_t(ds[g].rlen) + 1;
        }
        m.gmem_off.swap(off), m.gmembers.swap(mem);
    }
    const size_t M = m.gmembers.size();
    std::vector<IocGroupWork>& work = d.work;
    work.clear();
    for (size_t x = 0; x < G; ++x)
        for (int64_t row = 0; m.gmem_off[x + 1] > m.gmem_off[x] && row <= int64_t(gsegs[x].rlen); row += IOC_GROUP_PILE_ROWS)
            work.push_back(IocGroupWork{uint32_t(x), uint32_t(row)});
    if (work.size() > size_t(INT32_MAX)) return ioc_fail(c, IOC_ERR_CAPACITY, "the group tables have more than 2^31 - 1 blocks of rows");
    Arena l;
    const size_t o_gseg = l.take(G * sizeof(IocPileSeg)), o_work = l.take(work.size() * sizeof(IocGroupWork)), o_plane = l.take(np * 8),
                 o_goff = l.take((G + 1) * 4), o_gmem = l.take(M * 4), o_base = l.take(pd.base ? 0 : P),
                 o_slots = l.take(pd.slots ? 0 : size_t(IOC_PILE_INS_SLOTS) * P), o_weights = l.take(!weighted || pd.weights ? 0 : size_t(IOC_WEIGHT_PLANES) * P),
                 o_cols = l.take(size_t(d.n_rows) * sizeof(ioc_pileup_col)), o_wcols = l.take(weighted ? size_t(d.n_rows) * sizeof(ioc_pileup_col) : 0),
                 o_ins = l.take(size_t(d.n_rows) * sizeof(ioc_pileup_ins));  // (weighted: gwins)
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_gpile, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_gpile.p);
    auto up = [&](size_t o, const void* src, size_t b) { return b ? hipMemcpyAsync(p + o, src, b, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
    IOC_CHK(c, up(o_gseg, gsegs.data(), G * sizeof(IocPileSeg)));
    IOC_CHK(c, up(o_work, work.data(), work.size() * sizeof(IocGroupWork)));
    IOC_CHK(c, up(o_plane, pn.plane.data(), np * 8));
    IOC_CHK(c, up(o_goff, m.gmem_off.data(), (G + 1) * 4));
    IOC_CHK(c, up(o_gmem, m.gmembers.data(), M * 4));
    if (!pd.base) IOC_CHK(c, up(o_base, ph.base, P));
    if (!pd.slots) IOC_CHK(c, up(o_slots, ph.slots, size_t(IOC_PILE_INS_SLOTS) * P));
    if (weighted && !pd.weights) {
        IOC_CHK(c, up(o_weights, ph.wbase, P));
        IOC_CHK(c, up(o_weights + P, ph.wslots, size_t(IOC_PILE_INS_SLOTS) * P));
    }
    if (!pd.base) pd.base = p + o_base;  // (what does not lie on the device yet was uploaded)
    if (!pd.slots) pd.slots = p + o_slots;
    if (weighted && !pd.weights) pd.weights = p + o_weights;
    d.dev_gsegs = reinterpret_cast<const IocPileSeg*>(p + o_gseg), d.base = pd.base, d.slots = pd.slots;
    d.cols = reinterpret_cast<ioc_pileup_col*>(p + o_cols), d.ins = reinterpret_cast<ioc_pileup_ins*>(p + o_ins);
    IOC_CHK(c, hipMemsetAsync(p + o_cols, 0, l.size() - o_cols, c->stream));
    if (weighted) {
        d.ins = nullptr, d.wcols = reinterpret_cast<ioc_pileup_col*>(p + o_wcols), d.wins = reinterpret_cast<ioc_pileup_ins*>(p + o_ins);
        IOC_TRY(begin(t.ms_group_pile_weighted));
        IOC_CHK(c, iock_group_pile_weighted(c->stream, reinterpret_cast<const IocGroupWork*>(p + o_work), uint32_t(work.size()),
                                            reinterpret_cast<const IocPileSeg*>(p + o_gseg), uint32_t(G), reinterpret_cast<const uint32_t*>(p + o_goff),
                                            reinterpret_cast<const uint32_t*>(p + o_gmem), uint32_t(M), uint32_t(np), reinterpret_cast<const uint64_t*>(p + o_plane),
                                            pd.base, pd.slots, pd.weights, uint64_t(P), d.cols, d.wcols, d.wins, uint64_t(d.n_rows)));
        return end();
    }
    IOC_TRY(begin(t.ms_group_pile));
    IOC_CHK(c, iock_group_pile(c->stream, reinterpret_cast<const IocGroupWork*>(p + o_work), uint32_t(work.size()), reinterpret_cast<const IocPileSeg*>(p + o_gseg),
                               uint32_t(G), reinterpret_cast<const uint32_t*>(p + o_goff), reinterpret_cast<const uint32_t*>(p + o_gmem), uint32_t(M), uint32_t(np),
                               reinterpret_cast<const uint64_t*>(p + o_plane), pd.base, pd.slots, uint64_t(P), d.cols, d.ins, uint64_t(d.n_rows)));
    return end();
}

// k_read_correct over the plan's pairs: tables and frames lie on the device, the planes either do (dev) or are the host's and
// uploaded.  a_correct holds [segments][seg_of_pair][plane offsets][pair_len][out_off][records] and, uploaded, [base plane][slot
// planes].  The count pass and the scan run first; the one word that comes back then, out_off[pairs], is what a_call is reserved
// for — [sequence][qualities], as many bytes as were counted, not as the bound allows — and the write pass fills it.
int SinkRun::correct(const SinkPlan& pn, const int32_t* seg_of_pair, const uint8_t* d_frames, uint64_t frame_bytes, const ioc_pileup_col* d_cols,
                     const ioc_pileup_ins* d_ins, const Planes& ph, Planes pd, const CorrectOut& o)
{
    const size_t n = pn.segs.size(), np = pn.plane.size(), P = size_t(pn.plane_bytes);
    o.off[0] = 0;
    if (np == 0) return IOC_OK;
    Arena l;
    const size_t o_seg = l.take(n * sizeof(IocPileSeg)), o_sop = l.take(np * 4), o_plane = l.take(np * 8), o_len = l.take(np * 8), o_off = l.take((np + 1) * 8),
                 o_st = l.take(np * sizeof(ioc_correct_stats)), o_base = l.take(pd.base ? 0 : P), o_slots = l.take(pd.slots ? 0 : size_t(IOC_PILE_INS_SLOTS) * P);
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_correct, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_correct.p);
    auto up = [&](size_t at, const void* src, size_t b) { return b ? hipMemcpyAsync(p + at, src, b, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
    IOC_CHK(c, up(o_seg, pn.segs.data(), n * sizeof(IocPileSeg)));
    IOC_CHK(c, up(o_sop, seg_of_pair, np * 4));
    IOC_CHK(c, up(o_plane, pn.plane.data(), np * 8));
    if (!pd.base) IOC_CHK(c, up(o_base, ph.base, P));
    if (!pd.slots) IOC_CHK(c, up(o_slots, ph.slots, size_t(IOC_PILE_INS_SLOTS) * P));
    if (!pd.base) pd.base = p + o_base;  // (what does not lie on the device yet was uploaded)
    if (!pd.slots) pd.slots = p + o_slots;
    const IocReadCorrectDev v{reinterpret_cast<const IocPileSeg*>(p + o_seg), uint32_t(n), uint32_t(np), reinterpret_cast<const int32_t*>(p + o_sop),
                              reinterpret_cast<const uint64_t*>(p + o_plane), d_cols, d_ins, uint64_t(pn.n_rows), d_frames, frame_bytes, pd.base, pd.slots,
                              uint64_t(P), reinterpret_cast<int64_t*>(p + o_len), reinterpret_cast<ioc_correct_stats*>(p + o_st)};
    const ReadRule& k = o.rule;
    IOC_TRY(begin(t.ms_correct));
    IOC_CHK(c, iock_read_correct_count(c->stream, v, k.min_depth, k.min_alt, k.min_pct, k.max_run, reinterpret_cast<int64_t*>(p + o_off)));
    IOC_TRY(end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    settled();
    int64_t total = 0;
    IOC_TRY(copy_out({{&total, p + o_off + np * 8, 8}}));
    if (total < 0 || total > pn.correct_bound) return ioc_fail(c, IOC_ERR_HIP, "the read correction counted a length outside its bound");
    Arena w;
    const size_t o_seq = w.take(size_t(total)), o_qual = w.take(size_t(total));
    IOC_TRY(ioc_reserve(c, c->a_call, w.size()));
    uint8_t* q = static_cast<uint8_t*>(c->a_call.p);
    IOC_TRY(begin(t.ms_correct));
    IOC_CHK(c, iock_read_correct_emit(c->stream, v, k.min_depth, k.min_alt, k.min_pct, k.max_run, reinterpret_cast<const int64_t*>(p + o_off), q + o_seq,
                                      q + o_qual, uint64_t(total)));
    IOC_TRY(end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    settled();
    return copy_out({{o.off, p + o_off, (np + 1) * 8}, {o.stats, p + o_st, np * sizeof(ioc_correct_stats)}, {o.seq, q + o_seq, size_t(total)},
                     {o.qual, q + o_qual, size_t(total)}});
}

// groups pile -> iso correct -> copy-out: every pair held against the tables of its own isoform.  k_group_pile piles the G tables of
// the groups and one more per segment over all of its pairs where some pair is held against it (groups_pile, all_below); the member counts it made its lists from say
// which table a pair takes (iso_uses_group), a word a pair.  The planes lie on the device (dev, dev_long) or are the host's and
// uploaded; the reads lie in the pool, pair i's q_len[i] bytes from q_off[i] on.  a_correct holds [table][plane offsets][q_off]
// [q_len][pair_len][out_off][records] and, uploaded, [length plane][position plane] (the base and slot planes: where groups_pile has them).  The
// count pass and the scan run first; the one word that comes back then, out_off[pairs], is what a_call is reserved for, and the
// write pass fills it.
int SinkRun::iso_correct(const SinkPlan& pn, const int32_t* seg_of_pair, const int32_t* group, const int32_t* n_groups, const uint8_t* d_frames, uint64_t frame_bytes,
                         const Planes& ph, Planes pd, const LongPlanes& lh, LongPlanes ld, const std::vector<uint64_t>& q_off, const std::vector<uint32_t>& q_len,
                         const IsoCorrectOut& o)
{
    const size_t n = pn.segs.size(), np = pn.plane.size(), P = size_t(pn.plane_bytes);
    o.off[0] = 0;
    if (np == 0) return IOC_OK;
    GroupPiled g;
    IOC_TRY(groups_pile(pn, seg_of_pair, group, n_groups, ph, pd, g, /*weighted*/ false, /*all_below*/ o.rule.min_depth));
    const GroupMemberLists& m = g.lists;
    const uint32_t G = m.gseg_off[n];
    std::vector<uint32_t> table(np);
    for (size_t i = 0; i < np; ++i) {
        const size_t s = size_t(seg_of_pair[i]);
        const bool in_group = group[i] >= 0 && group[i] < n_groups[s];
        const uint32_t x = in_group ? m.gseg_off[s] + uint32_t(group[i]) : 0u;
        table[i] = in_group && iso_uses_group(group[i], m.gmem_off[x + 1] - m.gmem_off[x], o.rule.min_depth) ? x : G + uint32_t(s);
    }
    Arena l;
    const size_t o_tab = l.take(np * 4), o_plane = l.take(np * 8), o_qoff = l.take(np * 8), o_qlen = l.take(np * 4), o_len = l.take(np * 8), o_off = l.take((np + 1) * 8),
                 o_st = l.take(np * sizeof(ioc_iso_correct_stats)), o_ilen = l.take(ld.ilen ? 0 : P), o_qpos = l.take(ld.qpos ? 0 : 4 * P);
    IOC_TRY(ioc_reserve(c, c->a_correct, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_correct.p);
    auto up = [&](size_t at, const void* src, size_t b) { return b ? hipMemcpyAsync(p + at, src, b, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
    IOC_CHK(c, up(o_tab, table.data(), np * 4));
    IOC_CHK(c, up(o_plane, pn.plane.data(), np * 8));
    IOC_CHK(c, up(o_qoff, q_off.data(), np * 8));
    IOC_CHK(c, up(o_qlen, q_len.data(), np * 4));
    if (!ld.ilen) IOC_CHK(c, up(o_ilen, lh.ilen, P));
    if (!ld.qpos) IOC_CHK(c, up(o_qpos, lh.qpos, 4 * P));
    if (!ld.ilen) ld.ilen = p + o_ilen;  // (what does not lie on the device yet was uploaded)
    if (!ld.qpos) ld.qpos = reinterpret_cast<const uint32_t*>(p + o_qpos);
    const IocIsoCorrectDev v{g.dev_gsegs, uint32_t(g.gsegs.size()), G, uint32_t(np), reinterpret_cast<const uint32_t*>(p + o_tab),
                             reinterpret_cast<const uint64_t*>(p + o_plane), g.cols, g.ins, uint64_t(g.n_rows), d_frames, frame_bytes, g.base, g.slots, ld.ilen, ld.qpos,
                             uint64_t(P), static_cast<const uint8_t*>(c->a_pool.p), uint64_t(c->aln_offs.empty() ? 0 : c->aln_offs.back()),
                             reinterpret_cast<const uint64_t*>(p + o_qoff), reinterpret_cast<const uint32_t*>(p + o_qlen), reinterpret_cast<int64_t*>(p + o_len),
                             reinterpret_cast<ioc_iso_correct_stats*>(p + o_st)};
    const ReadRule& k = o.rule;
    int64_t bound = pn.correct_bound;
    for (const uint32_t len : q_len) bound += len;
    IOC_TRY(begin(t.ms_iso_correct));
    IOC_CHK(c, iock_iso_correct_count(c->stream, v, k.min_depth, k.min_alt, k.min_pct, k.max_run, reinterpret_cast<int64_t*>(p + o_off)));
    IOC_TRY(end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    settled();
    int64_t total = 0;
    IOC_TRY(copy_out({{&total, p + o_off + np * 8, 8}}));
    if (total < 0 || total > bound) return ioc_fail(c, IOC_ERR_HIP, "the read correction by isoform counted a length outside its bound");
    Arena w;
    const size_t o_seq = w.take(size_t(total)), o_qual = w.take(size_t(total));
    IOC_TRY(ioc_reserve(c, c->a_call, w.size()));
    uint8_t* q = static_cast<uint8_t*>(c->a_call.p);
    IOC_TRY(begin(t.ms_iso_correct));
    IOC_CHK(c, iock_iso_correct_emit(c->stream, v, k.min_depth, k.min_alt, k.min_pct, k.max_run, reinterpret_cast<const int64_t*>(p + o_off), q + o_seq, q + o_qual,
                                     uint64_t(total)));
    IOC_TRY(end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    settled();
    return copy_out({{o.off, p + o_off, (np + 1) * 8}, {o.stats, p + o_st, np * sizeof(ioc_iso_correct_stats)}, {o.seq, q + o_seq, size_t(total)},
                     {o.qual, q + o_qual, size_t(total)}});
}

// The kernels of ioc_read_blocks.hip over the plan's pairs: the base planes lie on the device (dev_base) or are the host's and
// uploaded.  a_blocks holds the host's tables [segments][seg_of_pair][plane offsets][mem_off][members][pair_word][seg_word][word_seg]
// [block_base], the kernels' own [covered][deleted][long gaps][variable rows][masks][flags][row table][block slots][read records]
// [segment records] and, uploaded, [base plane].  The segment records come back first: they say how many of a segment's slots are
// blocks, and the blocks are packed on the host.
int SinkRun::blocks(const SinkPlan& pn, const int32_t* seg_of_pair, const uint8_t* host_base, const uint8_t* dev_base, const BlocksOut& o, BlocksDev* where)
{
    const size_t n = pn.segs.size(), np = pn.plane.size(), B = size_t(pn.plane_bytes);
    const BlocksTables bt = blocks_tables(pn, seg_of_pair, o.rule.max_blocks);
    const MemberLists m = member_lists(n, np, seg_of_pair);
    const size_t P = bt.P, T = bt.T, slots = size_t(bt.block_base[n]);
    Arena l;
    const size_t o_seg = l.take(n * sizeof(IocPileSeg)), o_sop = l.take(np * 4), o_plane = l.take(np * 8), o_moff = l.take((n + 1) * 4), o_mem = l.take(np * 4),
                 o_pw = l.take(np * 8), o_sw = l.take((n + 1) * 8), o_ws = l.take(T * 4), o_bb = l.take((n + 1) * 8), tables = l.size();
    const size_t o_cov = l.take(P * 8), o_del = l.take(P * 8), o_gap = l.take(P * 8), o_var = l.take(T * 8), o_mask = l.take(np * 8), o_flags = l.take(np),
                 o_rows = l.take(size_t(pn.n_rows) * sizeof(ioc_block_row)), o_blk = l.take(slots * sizeof(ioc_pile_block)),
                 o_reads = l.take(np * sizeof(ioc_read_blocks)), o_rec = l.take(n * sizeof(ioc_blocks_seg)), o_end = l.size(),
                 o_base = l.take(dev_base ? 0 : B);
    std::vector<uint8_t> stage(tables, 0);
    auto put = [&](size_t at, const void* src, size_t b) { if (b) memcpy(stage.data() + at, src, b); };
    put(o_seg, pn.segs.data(), n * sizeof(IocPileSeg)), put(o_sop, seg_of_pair, np * 4), put(o_plane, pn.plane.data(), np * 8);
    put(o_moff, m.mem_off.data(), (n + 1) * 4), put(o_mem, m.members.data(), np * 4), put(o_pw, bt.pair_word.data(), np * 8);
    put(o_sw, bt.seg_word.data(), (n + 1) * 8), put(o_ws, bt.word_seg.data(), T * 4), put(o_bb, bt.block_base.data(), (n + 1) * 8);
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_blocks, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_blocks.p);
    IOC_CHK(c, hipMemcpyAsync(p, stage.data(), tables, hipMemcpyHostToDevice, c->stream));
    if (!dev_base && B) IOC_CHK(c, hipMemcpyAsync(p + o_base, host_base, B, hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemsetAsync(p + o_blk, 0, o_end - o_blk, c->stream));  // (the block slots and both kinds of record)
    auto u64p = [&](size_t at) { return reinterpret_cast<unsigned long long*>(p + at); };
    const IocReadBlocksDev v{reinterpret_cast<const IocPileSeg*>(p + o_seg), uint32_t(n), uint32_t(np), reinterpret_cast<const int32_t*>(p + o_sop),
                             reinterpret_cast<const uint64_t*>(p + o_plane), dev_base ? dev_base : p + o_base, uint64_t(B),
                             reinterpret_cast<const uint32_t*>(p + o_moff), reinterpret_cast<const uint32_t*>(p + o_mem),
                             reinterpret_cast<const uint64_t*>(p + o_pw), reinterpret_cast<const uint64_t*>(p + o_sw), reinterpret_cast<const int32_t*>(p + o_ws),
                             reinterpret_cast<const int64_t*>(p + o_bb), uint64_t(P), uint64_t(T), uint64_t(pn.n_rows), uint64_t(slots), u64p(o_cov), u64p(o_del),
                             u64p(o_gap), u64p(o_var), u64p(o_mask), p + o_flags, reinterpret_cast<ioc_block_row*>(p + o_rows),
                             reinterpret_cast<ioc_pile_block*>(p + o_blk), reinterpret_cast<ioc_read_blocks*>(p + o_reads), reinterpret_cast<ioc_blocks_seg*>(p + o_rec)};
    if (where) *where = BlocksDev{v.reads, v.mask};
    const BlocksRule& k = o.rule;
    IOC_TRY(begin(t.ms_blocks));
    IOC_CHK(c, iock_read_blocks(c->stream, v, k.min_gap, k.min_depth, k.min_alt, k.min_pct, k.min_block, k.max_blocks));
    IOC_TRY(end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    settled();
    std::vector<ioc_blocks_seg> rec(n);
    std::vector<ioc_pile_block> slot(slots);
    IOC_TRY(copy_out({{rec.data(), p + o_rec, n * sizeof(ioc_blocks_seg)}, {slot.data(), p + o_blk, slots * sizeof(ioc_pile_block)}}));
    for (size_t g = 0; g < n; ++g)
        if (rec[g].n_blocks < 0 || rec[g].n_blocks > bt.block_base[g + 1] - bt.block_base[g])
            return ioc_fail(c, IOC_ERR_HIP, "the block search returned a count outside its bound");
    pack_kept_slots(slot, bt.block_base.data(), n, [&](size_t g) { return rec[g].n_blocks; }, o.blocks, o.block_off);
    std::copy(rec.begin(), rec.end(), o.seg);
    return copy_out({{o.reads, p + o_reads, np * sizeof(ioc_read_blocks)}, {o.rows, p + o_rows, size_t(pn.n_rows) * sizeof(ioc_block_row)}});
}

// The kernels of ioc_read_inserts.hip over the plan's pairs: the base and the length planes lie on the device (dev_base, dev_ilen)
// or are the host's and uploaded; the block stage's words likewise, or there are none.  a_inserts holds the host's tables [segments]
// [seg_of_pair][plane offsets][mem_off][members][pair_word][seg_word][word_seg][site_base][slot_seg][pre_full], the kernels' own
// [spans][near][variable junctions][masks][flags][largest sums][row table][site slots][read records][segment records] and, uploaded, [base plane]
// [length plane][pre_key][pre_mask].  The segment records come back first and the sites are packed on the host, as the blocks are.
// Under IOC_TRACE every kernel is timed on its own (t.ms_inserts, in the order they run); otherwise ms_inserts[0] has all of them.
int SinkRun::inserts(const SinkPlan& pn, const int32_t* seg_of_pair, const uint8_t* host_base, const uint8_t* host_ilen, const uint8_t* dev_base,
                     const uint8_t* dev_ilen, const InsertsPre& pre, const InsertsOut& o)
{
    const size_t n = pn.segs.size(), np = pn.plane.size(), B = size_t(pn.plane_bytes);
    const BlocksTables bt = blocks_tables(pn, seg_of_pair, 1);  // (the words of a pair and of a segment are the block stage's)
    const MemberLists m = member_lists(n, np, seg_of_pair);
    std::vector<int64_t> site_base(n + 1, 0);
    for (size_t g = 0; g < n; ++g) site_base[g + 1] = site_base[g] + inserts_sites_most(pn.segs[g].rlen, o.rule.max_sites);
    const size_t P = bt.P, T = bt.T, slots = size_t(site_base[n]);
    const std::vector<int32_t> slot_seg = slot_owners(site_base.data(), n);
    const bool pre_host = pre.host_key != nullptr, pre_dev = pre.dev_key != nullptr, with_pre = pre_host || pre_dev;
    Arena l;
    const size_t o_seg = l.take(n * sizeof(IocPileSeg)), o_sop = l.take(np * 4), o_plane = l.take(np * 8), o_moff = l.take((n + 1) * 4), o_mem = l.take(np * 4),
                 o_pw = l.take(np * 8), o_sw = l.take((n + 1) * 8), o_ws = l.take(T * 4), o_sb = l.take((n + 1) * 8), o_ss = l.take(slots * 4),
                 o_pf = l.take(with_pre ? n * 8 : 0), tables = l.size();
    const size_t S = size_t(o.rule.max_sites);
    const size_t o_span = l.take(P * 8), o_near = l.take(P * 8), o_var = l.take(T * 8), o_mask = l.take(np * 8), o_flags = l.take(np), o_wmax = l.take(np * S * 2),
                 o_rows = l.take(size_t(pn.n_rows) * sizeof(ioc_insert_row)), o_sites = l.take(slots * sizeof(ioc_pile_insert)),
                 o_reads = l.take(np * sizeof(ioc_read_inserts)), o_rec = l.take(n * sizeof(ioc_inserts_seg)), o_end = l.size(),
                 o_base = l.take(dev_base ? 0 : B), o_ilen = l.take(dev_ilen ? 0 : B), o_pk = l.take(pre_host ? np * 8 : 0), o_pm = l.take(pre_host ? np * 8 : 0);
    std::vector<uint8_t> stage(tables, 0);
    auto put = [&](size_t at, const void* src, size_t b) { if (b) memcpy(stage.data() + at, src, b); };
    put(o_seg, pn.segs.data(), n * sizeof(IocPileSeg)), put(o_sop, seg_of_pair, np * 4), put(o_plane, pn.plane.data(), np * 8);
    put(o_moff, m.mem_off.data(), (n + 1) * 4), put(o_mem, m.members.data(), np * 4), put(o_pw, bt.pair_word.data(), np * 8);
    put(o_sw, bt.seg_word.data(), (n + 1) * 8), put(o_ws, bt.word_seg.data(), T * 4), put(o_sb, site_base.data(), (n + 1) * 8);
    put(o_ss, slot_seg.data(), slots * 4);
    if (with_pre) put(o_pf, pre.pre_full, n * 8);
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_inserts, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_inserts.p);
    IOC_CHK(c, hipMemcpyAsync(p, stage.data(), tables, hipMemcpyHostToDevice, c->stream));
    if (!dev_base && B) IOC_CHK(c, hipMemcpyAsync(p + o_base, host_base, B, hipMemcpyHostToDevice, c->stream));
    if (!dev_ilen && B) IOC_CHK(c, hipMemcpyAsync(p + o_ilen, host_ilen, B, hipMemcpyHostToDevice, c->stream));
    if (pre_host && np) {
        IOC_CHK(c, hipMemcpyAsync(p + o_pk, pre.host_key, np * 8, hipMemcpyHostToDevice, c->stream));
        IOC_CHK(c, hipMemcpyAsync(p + o_pm, pre.host_mask, np * 8, hipMemcpyHostToDevice, c->stream));
    }
    IOC_CHK(c, hipMemsetAsync(p + o_sites, 0, o_end - o_sites, c->stream));  // (the site slots and both kinds of record)
    auto u64p = [&](size_t at) { return reinterpret_cast<unsigned long long*>(p + at); };
    const IocReadInsertsDev v{reinterpret_cast<const IocPileSeg*>(p + o_seg), uint32_t(n), uint32_t(np), reinterpret_cast<const int32_t*>(p + o_sop),
                              reinterpret_cast<const uint64_t*>(p + o_plane), dev_base ? dev_base : p + o_base, dev_ilen ? dev_ilen : p + o_ilen, uint64_t(B),
                              reinterpret_cast<const uint32_t*>(p + o_moff), reinterpret_cast<const uint32_t*>(p + o_mem),
                              reinterpret_cast<const uint64_t*>(p + o_pw), reinterpret_cast<const uint64_t*>(p + o_sw), reinterpret_cast<const int32_t*>(p + o_ws),
                              reinterpret_cast<const int64_t*>(p + o_sb), reinterpret_cast<const int32_t*>(p + o_ss), uint64_t(P), uint64_t(T), uint64_t(pn.n_rows),
                              uint64_t(slots), pre_dev ? pre.dev_key : pre_host ? u64p(o_pk) : nullptr, pre_dev ? pre.dev_mask : pre_host ? u64p(o_pm) : nullptr,
                              with_pre ? u64p(o_pf) : nullptr, pre_dev ? pre.dev_key_stride : 1u, pre_dev ? pre.dev_mask_stride : 1u, u64p(o_span), u64p(o_near),
                              u64p(o_var), u64p(o_mask), p + o_flags, reinterpret_cast<uint16_t*>(p + o_wmax), uint32_t(S), uint64_t(np * S),
                              reinterpret_cast<ioc_insert_row*>(p + o_rows), reinterpret_cast<ioc_pile_insert*>(p + o_sites),
                              reinterpret_cast<ioc_read_inserts*>(p + o_reads), reinterpret_cast<ioc_inserts_seg*>(p + o_rec)};
    const InsertsRule& k = o.rule;
    KernelTimes each;
    IOC_TRY(each.create(c, IOC_READ_INSERTS_KERNELS));
    IOC_TRY(begin(t.ms_inserts[0], !each.on()));
    IOC_CHK(c, iock_read_inserts(c->stream, v, k.min_ins, k.slack, k.min_depth, k.min_alt, k.min_pct, k.max_sites, each.events()));
    IOC_TRY(end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    settled();
    each.add_to(t.ms_inserts);
    std::vector<ioc_inserts_seg> rec(n);
    std::vector<ioc_pile_insert> slot(slots);
    IOC_TRY(copy_out({{rec.data(), p + o_rec, n * sizeof(ioc_inserts_seg)}, {slot.data(), p + o_sites, slots * sizeof(ioc_pile_insert)}}));
    for (size_t g = 0; g < n; ++g)
        if (rec[g].n_sites < 0 || rec[g].n_sites > site_base[g + 1] - site_base[g])
            return ioc_fail(c, IOC_ERR_HIP, "the search for insertion sites returned a count outside its bound");
    pack_kept_slots(slot, site_base.data(), n, [&](size_t g) { return rec[g].n_sites; }, o.sites, o.site_off);
    std::copy(rec.begin(), rec.end(), o.seg);
    return copy_out({{o.reads, p + o_reads, np * sizeof(ioc_read_inserts)}, {o.rows, p + o_rows, size_t(pn.n_rows) * sizeof(ioc_insert_row)}});
}

// The kernels of ioc_read_ends.hip over the plan's pairs: the extents are the host's and uploaded; pre_group likewise (host_pre), or
// lies on the device (dev_pre, a word every dev_pre_stride words), or there is none.  a_rends holds the host's tables [segments]
// [seg_of_pair][mem_off][members][seg_word][word_seg][site_base][slot_unit][var_base][extents][pre_group], what the kernels add into
// and what comes back packed on the host, set to 0 — [histograms][N per segment][site slots][variant slots][segment records] — and the
// kernels' own [start rows][stop rows][keys][same][flags][read records][row table].  The segment records come back first and the
// sites and variants are packed on the host, as the blocks are.  Under IOC_TRACE every kernel is timed on its own (t.ms_ends, in the
// order they run); otherwise ms_ends[0] has all of them.
int SinkRun::ends(const SinkPlan& pn, const int32_t* seg_of_pair, const ioc_read_extent* extents, const int32_t* host_pre, const int32_t* dev_pre,
                  uint32_t dev_pre_stride, const EndsOut& o)
{
    const size_t n = pn.segs.size(), np = pn.plane.size();
    const MemberLists m = member_lists(n, np, seg_of_pair);
    const SegWordTable sw = seg_word_table(pn.segs);  // (the words of a segment are the block stage's)
    std::vector<int64_t> site_base(2 * n + 1, 0), var_base(n + 1, 0);
    for (size_t g = 0; g < n; ++g) {
        site_base[2 * g + 1] = site_base[2 * g] + ends_sites_most(pn.segs[g].rlen, o.rule.max_sites);
        site_base[2 * g + 2] = site_base[2 * g + 1] + ends_sites_most(pn.segs[g].rlen, o.rule.max_sites);
        var_base[g + 1] = var_base[g] + ends_variants_most(int64_t(m.mem_off[g + 1] - m.mem_off[g]), o.rule.max_variants);
    }
    const size_t T = sw.T, slots = size_t(site_base[2 * n]), vslots = size_t(var_base[n]), R = size_t(pn.n_rows);
    const std::vector<int32_t> slot_unit = slot_owners(site_base.data(), 2 * n);
    Arena l;
    const size_t o_seg = l.take(n * sizeof(IocPileSeg)), o_sop = l.take(np * 4), o_moff = l.take((n + 1) * 4), o_mem = l.take(np * 4), o_sw = l.take((n + 1) * 8),
                 o_ws = l.take(T * 4), o_sb = l.take((2 * n + 1) * 8), o_su = l.take(slots * 4), o_vb = l.take((n + 1) * 8),
                 o_ext = l.take(np * sizeof(ioc_read_extent)), o_pre = l.take(host_pre ? np * 4 : 0), tables = l.size();
    const size_t o_hist = l.take(R * sizeof(uint2)), o_part = l.take(n * 4), o_sites = l.take(slots * sizeof(ioc_end_site)),
                 o_vars = l.take(vslots * sizeof(ioc_end_variant)), o_rec = l.take(n * sizeof(ioc_ends_seg)), o_zend = l.size();
    const size_t o_bs = l.take(T * 8), o_be = l.take(T * 8), o_key = l.take(np * 8), o_same = l.take(np * 4), o_flags = l.take(np),
                 o_reads = l.take(np * sizeof(ioc_read_ends)), o_rows = l.take(o.rows ? R * sizeof(ioc_end_row) : 0);
    std::vector<uint8_t> stage(tables, 0);
    auto put = [&](size_t at, const void* src, size_t b) { if (b) memcpy(stage.data() + at, src, b); };
    put(o_seg, pn.segs.data(), n * sizeof(IocPileSeg)), put(o_sop, seg_of_pair, np * 4), put(o_moff, m.mem_off.data(), (n + 1) * 4);
    put(o_mem, m.members.data(), np * 4), put(o_sw, sw.seg_word.data(), (n + 1) * 8), put(o_ws, sw.word_seg.data(), T * 4);
    put(o_sb, site_base.data(), (2 * n + 1) * 8), put(o_su, slot_unit.data(), slots * 4), put(o_vb, var_base.data(), (n + 1) * 8);
    put(o_ext, extents, np * sizeof(ioc_read_extent));
    if (host_pre) put(o_pre, host_pre, np * 4);
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_rends, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_rends.p);
    IOC_CHK(c, hipMemcpyAsync(p, stage.data(), tables, hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemsetAsync(p + o_hist, 0, o_zend - o_hist, c->stream));  // (the histograms, N, the slots and the segment records)
    auto u64p = [&](size_t at) { return reinterpret_cast<unsigned long long*>(p + at); };
    const IocReadEndsDev v{reinterpret_cast<const IocPileSeg*>(p + o_seg), uint32_t(n), uint32_t(np), reinterpret_cast<const int32_t*>(p + o_sop),
                           reinterpret_cast<const ioc_read_extent*>(p + o_ext), dev_pre ? dev_pre : host_pre ? reinterpret_cast<const int32_t*>(p + o_pre) : nullptr,
                           dev_pre ? dev_pre_stride : 1u, reinterpret_cast<const uint32_t*>(p + o_moff), reinterpret_cast<const uint32_t*>(p + o_mem),
                           reinterpret_cast<const uint64_t*>(p + o_sw), reinterpret_cast<const int32_t*>(p + o_ws), reinterpret_cast<const int64_t*>(p + o_sb),
                           reinterpret_cast<const int64_t*>(p + o_vb), reinterpret_cast<const int32_t*>(p + o_su), uint64_t(T), uint64_t(R), uint64_t(slots),
                           uint64_t(vslots), reinterpret_cast<uint2*>(p + o_hist), reinterpret_cast<uint32_t*>(p + o_part), u64p(o_bs), u64p(o_be), u64p(o_key),
                           reinterpret_cast<uint32_t*>(p + o_same), p + o_flags, o.rows ? reinterpret_cast<ioc_end_row*>(p + o_rows) : nullptr,
                           reinterpret_cast<ioc_end_site*>(p + o_sites), reinterpret_cast<ioc_end_variant*>(p + o_vars),
                           reinterpret_cast<ioc_read_ends*>(p + o_reads), reinterpret_cast<ioc_ends_seg*>(p + o_rec)};
    const EndsRule& k = o.rule;
    KernelTimes each;
    IOC_TRY(each.create(c, IOC_READ_ENDS_KERNELS));
    IOC_TRY(begin(t.ms_ends[0], !each.on()));
    IOC_CHK(c, iock_read_ends(c->stream, v, k.slack, k.min_over, k.min_depth, k.min_alt, k.min_pct, k.max_sites, k.max_variants, each.events()));
    IOC_TRY(end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    settled();
    each.add_to(t.ms_ends);
    std::vector<ioc_ends_seg> rec(n);
    std::vector<ioc_end_site> slot(slots);
    std::vector<ioc_end_variant> vslot(vslots);
    IOC_TRY(copy_out({{rec.data(), p + o_rec, n * sizeof(ioc_ends_seg)}, {slot.data(), p + o_sites, slots * sizeof(ioc_end_site)},
                      {vslot.data(), p + o_vars, vslots * sizeof(ioc_end_variant)}}));
    for (size_t g = 0; g < n; ++g)
        if (rec[g].n_starts < 0 || rec[g].n_starts > site_base[2 * g + 1] - site_base[2 * g] || rec[g].n_stops < 0 ||
            rec[g].n_stops > site_base[2 * g + 2] - site_base[2 * g + 1] || rec[g].n_variants < 0 || rec[g].n_variants > var_base[g + 1] - var_base[g])
            return ioc_fail(c, IOC_ERR_HIP, "the search for ends returned a count outside its bound");
    pack_kept_slots(slot, site_base.data(), 2 * n, [&](size_t u) { return u & 1 ? rec[u / 2].n_stops : rec[u / 2].n_starts; }, o.sites, o.site_off);
    pack_kept_slots(vslot, var_base.data(), n, [&](size_t g) { return rec[g].n_variants; }, o.variants, o.var_off);
    std::copy(rec.begin(), rec.end(), o.seg);
    return copy_out({{o.reads, p + o_reads, np * sizeof(ioc_read_ends)}, {o.rows, p + o_rows, R * sizeof(ioc_end_row)}});
}

}  // namespace

// (two weak instantiations the symbol list has held since the optimiser left them out of line in the function that carried four of
// the block family's calls: instantiated here, so that the list does not hang on what is inlined where)
template void std::vector<int64_t>::push_back(const int64_t&);
template void std::vector<uint32_t>::push_back(uint32_t&&);

// (pile_call_bound, pile_call_device, group_polish_ok, group_polish_device, pileup_call_tables and align_pairs_polish stand inside
// extern "C", where they have always stood: there a function has external linkage even in an unnamed namespace, and these plain
// names are part of the library's symbol list — which is why the call stage and the group polish are no members of SinkRun)
extern "C" {
namespace {
int64_t pile_call_bound(const std::vector<IocPileSeg>& segs) { return ::pile_call_bound(segs); }  // (the name alone: ioc_sink_plan.h has the function)

// The call stage: the call kernels over tables that lie on the device (n_rows records each), and what they made copied back.  a_call
// holds [segments][seg_len][out_off][records][sequence][qualities] — reserved here, so whatever a site search left in a_call is gone
// from here on.  d_gate (the weighted call): d_cols / d_ins are weights, this the counts; else NULL.
int pile_call_device(SinkRun& r, const std::vector<IocPileSeg>& segs, const uint8_t* d_frames, uint64_t frame_bytes, const CallOut& o, const ioc_pileup_col* d_cols,
                     const ioc_pileup_ins* d_ins, const ioc_pileup_col* d_gate, int64_t n_rows)
{
    ioc_ctx* const c = r.c;
    const size_t n = segs.size(), bound = size_t(::pile_call_bound(segs));
    Arena l;
    const size_t o_seg = l.take(n * sizeof(IocPileSeg)), o_len = l.take(n * 8), o_off = l.take((n + 1) * 8), o_st = l.take(n * sizeof(ioc_polish_stats)),
                 o_seq = l.take(bound), o_qual = l.take(bound);
    IOC_TRY(ioc_reserve(c, c->a_call, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_call.p);
    IOC_CHK(c, hipMemcpyAsync(p + o_seg, segs.data(), n * sizeof(IocPileSeg), hipMemcpyHostToDevice, c->stream));
    IOC_TRY(r.begin(r.t.ms_call));
    if (d_gate)
        IOC_CHK(c, iock_pile_call_weighted(c->stream, reinterpret_cast<const IocPileSeg*>(p + o_seg), uint32_t(n), d_gate, d_cols, d_ins,
                                           uint64_t(n_rows), d_frames, frame_bytes, o.min_depth, reinterpret_cast<int64_t*>(p + o_len),
                                           reinterpret_cast<ioc_polish_stats*>(p + o_st), reinterpret_cast<int64_t*>(p + o_off), p + o_seq,
                                           p + o_qual, uint64_t(bound)));
    else
        IOC_CHK(c, iock_pile_call(c->stream, reinterpret_cast<const IocPileSeg*>(p + o_seg), uint32_t(n), d_cols, d_ins, uint64_t(n_rows), d_frames,
                                  frame_bytes, o.min_depth, reinterpret_cast<int64_t*>(p + o_len), reinterpret_cast<ioc_polish_stats*>(p + o_st),
                                  reinterpret_cast<int64_t*>(p + o_off), p + o_seq, p + o_qual, uint64_t(bound)));
    IOC_TRY(r.end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    r.settled();
    IOC_TRY(r.copy_out({{o.off, p + o_off, (n + 1) * 8}}));
    const int64_t len = o.off[n];
    if (len < 0 || size_t(len) > bound) return ioc_fail(c, IOC_ERR_HIP, "the consensus call returned a length outside its bound");
    return r.copy_out({{o.stats, p + o_st, n * sizeof(ioc_polish_stats)}, {o.seq, p + o_seq, size_t(len)}, {o.qual, p + o_qual, size_t(len)}});
}

// what a group polish refuses once its segments are known
int group_polish_ok(ioc_ctx* c, const std::string& who, const GroupPolish& gp, const std::vector<IocPileSeg>& ds)
{
    for (size_t g = 0; g < ds.size(); ++g)
        if (pile_call_most(ds[g].rlen) > INT32_MAX)  // (the record's out_len, the kernels' byte counts)
            return ioc_fail(c, IOC_ERR_CAPACITY, who + ": segment " + std::to_string(g) + " may call more than 2^31 - 1 bytes");
    return call_room_ok(c, who, gp.call, 2 * ::pile_call_bound(ds));
}

// group pile -> call -> copy-out: the consensus of both groups of every segment (frames in d_frames), the group tables where asked for
int group_polish_device(SinkRun& r, const GroupPolish& gp, const SinkPlan& p, const uint8_t* d_frames, uint64_t frame_bytes, const int32_t* seg_of_pair, const Planes& host,
                        const Planes& dev)
{
    GroupPiled g;
    IOC_TRY(r.group_pile(p, seg_of_pair, host, dev, g));
    IOC_TRY(pile_call_device(r, g.gsegs, d_frames, frame_bytes, gp.call, g.cols, g.ins, nullptr, 2 * p.n_rows));
    return r.copy_out({{gp.out_gcols, g.cols, size_t(2 * p.n_rows) * sizeof(ioc_pileup_col)}, {gp.out_gins, g.ins, size_t(2 * p.n_rows) * sizeof(ioc_pileup_ins)}});
}

// ioc_pileup_call (wcols NULL: cols / ins are called by majority) and ioc_pileup_call_weighted (cols gates, wcols / ins decide):
// upload -> call.  The tables are called where they lie then (ioc_pile_call.hip); the frames travel as one pool of bytes.
int pileup_call_tables(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, const ioc_pileup_col* cols,
                       const ioc_pileup_col* wcols, const ioc_pileup_ins* ins, const CallOut& o)
{
    if (!c || n_segs < 0 || !o.ok() || (n_segs > 0 && (!rlen || !frame_off || !cols || !ins))) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen("ioc_pileup_call", n_segs, rlen, frames, frame_off, 0, nullptr, nullptr, PLAN_REFUSE_CALLED)) return ioc_fail(c, st, p.msg);
    IOC_TRY(call_room_ok(c, "ioc_pileup_call", o, ::pile_call_bound(p.segs)));
    o.off[0] = 0;
    if (n_segs == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    const size_t b_cols = size_t(p.n_rows) * sizeof(ioc_pileup_col), b_ins = size_t(p.n_rows) * sizeof(ioc_pileup_ins);
    IOC_TRY(ioc_reserve(c, c->a_pile, b_cols));
    IOC_TRY(ioc_reserve(c, c->a_pile_ins, b_ins));
    DevBuf d_frames;
    IOC_TRY(ioc_alloc(c, d_frames, size_t(p.frame_bytes)));
    IOC_CHK(c, hipMemcpyAsync(c->a_pile.p, cols, b_cols, hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemcpyAsync(c->a_pile_ins.p, ins, b_ins, hipMemcpyHostToDevice, c->stream));
    if (wcols) {
        IOC_TRY(ioc_reserve(c, c->a_pile_w, b_cols));
        IOC_CHK(c, hipMemcpyAsync(c->a_pile_w.p, wcols, b_cols, hipMemcpyHostToDevice, c->stream));
    }
    if (p.frame_bytes > 0) IOC_CHK(c, hipMemcpyAsync(d_frames.p, frames, size_t(p.frame_bytes), hipMemcpyHostToDevice, c->stream));
    SinkRun r{c};
    IOC_TRY(pile_call_device(r, p.segs, static_cast<const uint8_t*>(d_frames.p), uint64_t(p.frame_bytes), o, wcols ? c->a_pile_w.as<ioc_pileup_col>() : c->a_pile.as<ioc_pileup_col>(),
                   c->a_pile_ins.as<ioc_pileup_ins>(), wcols ? c->a_pile.as<ioc_pileup_col>() : nullptr, p.n_rows));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   consensus call: %d segments, %lld rows, %lld bytes called, k_pile_call%s %.3f ms\n", n_segs, (long long)p.n_rows,
                (long long)o.off[n_segs], wcols ? "<weighted>" : "", r.t.ms_call);
    return IOC_OK;
}

// ioc_align_pairs_polish: pile -> call -> copy-out.  ioc_align_pairs_pileup with the second table beside the first, and the call kernels
// over both where they lie: what comes back is the called bytes (at most 7 per row), not the tables, unless they are asked for.  weighted
// (ioc_align_pairs_polish_weighted): the counts go into the first table, the weights into [wcols][wins] of a_pile_w; out_ins is then out_wins.
int align_pairs_polish(ioc_ctx* c, const AlnCall& a, ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair,
                       const CallOut& o, ioc_pileup_col* out_cols, ioc_pileup_ins* out_ins, bool weighted, ioc_pileup_col* out_wcols)
{
    if (!c || a.n_pairs < 0 || n_segs < 0 || !o.ok() || (a.n_pairs > 0 && (!a.pairs || !seg_of_pair)) || (n_segs > 0 && (!segs || !o.stats))) return IOC_ERR_ARG;
    if (weighted && !c->aln_qual_set) return ioc_fail(c, IOC_ERR_ARG, "ioc_align_pairs_polish_weighted: no qualities are set for the current pool (ioc_align_set_pool_qual)");
    SinkPlan p;
    if (int st = p.from_pool("ioc_align_pairs_polish", c->aln_offs, n_segs, segs, a.n_pairs, a.pairs, seg_of_pair, 0, 0)) return ioc_fail(c, st, p.msg);
    IOC_TRY(call_room_ok(c, "ioc_align_pairs_polish", o, ::pile_call_bound(p.segs)));
    for (int32_t i = 0; i < a.n_pairs && out_stats; ++i) out_stats[i] = ioc_aln_stats{};
    o.off[0] = 0;
    if (n_segs == 0) return a.run(c, nullptr);
    SinkRun r{c};
    PiledDev d;
    IOC_TRY(r.pile(a, weighted ? PileKind::weighted : PileKind::ins, out_stats, p.row_base.data(), p.n_rows, nullptr, 0, PileProject{}, d));
    IOC_TRY(pile_call_device(r, p.segs, static_cast<const uint8_t*>(c->a_pool.p), uint64_t(c->aln_offs.back()), o, weighted ? d.wcols : d.cols, weighted ? d.wins : d.ins,
                   weighted ? d.cols : nullptr, p.n_rows));
    const size_t b_cols = size_t(p.n_rows) * sizeof(ioc_pileup_col);
    IOC_TRY(r.copy_out({{out_cols, d.cols, b_cols}, {out_wcols, d.wcols, b_cols}, {out_ins, weighted ? d.wins : d.ins, size_t(p.n_rows) * sizeof(ioc_pileup_ins)}}));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: polish: %d segments, %lld rows, %.3f MB (called bytes, records, lengths%s%s) copied from the device in %.3f ms, k_ops_pileup<%s> %.3f ms, k_pile_call%s %.3f ms%s\n",
                n_segs, (long long)p.n_rows, double(r.t.copied) * 1e-6, out_cols || out_ins || out_wcols ? ", tables" : "", out_stats ? ", statistics" : "", r.t.ms_copy,
                weighted ? "weighted" : "ins", r.t.ms_pileup, weighted ? "<weighted>" : "", r.t.ms_call, out_stats ? (", k_ops_stats " + std::to_string(r.t.ms_stats) + " ms").c_str() : "");
    return IOC_OK;
}

// the segments of a call over the pool, and where its sites and alleles go (ioc_align_pairs_alleles' arguments behind the rule)
struct AllelesCall {
    int32_t n_segs;
    const ioc_polish_seg* segs;
    const int32_t* seg_of_pair;
    ioc_pile_site* out_sites;
    uint8_t* out_alleles;  // (may be NULL with a split: the alleles stay on the device)
    ioc_pileup_col* out_cols;
    int64_t sites_cap, alleles_cap;
    int64_t *site_off, *n_found, *allele_off;
};

// ioc_align_pairs_alleles: pile -> sites -> alleles -> [split] -> [group pile -> call] -> copy-out.  ioc_align_pairs_pileup into
// the rows of the segments, with every pair projected beside it, and the site kernels over the table and the planes where they
// lie: what comes back is the sites and one byte per (pair, kept site of its segment).  `split` (ioc_align_pairs_split): it runs
// behind k_site_alleles, out_alleles is optional; `gp` (ioc_align_pairs_split_polish, with `split`): both groups of every segment are called.
static int align_pairs_alleles(const std::string& who, ioc_ctx* c, const AlnCall& a, ioc_aln_stats* out_stats, const SitesRule& rule, const AllelesCall& o,
                        const SplitCall* split, const GroupPolish* gp)
{
    const int32_t n_pairs = a.n_pairs, n_segs = o.n_segs;
    if (gp && (!split || !gp->call.ok())) return IOC_ERR_ARG;
    if (split && (!split->ok() || (n_pairs > 0 && !split->out_group) || (n_segs > 0 && !split->out_seg))) return IOC_ERR_ARG;
    if (!c || n_pairs < 0 || n_segs < 0 || !rule.ok() || !o.site_off || !o.allele_off || o.sites_cap < 0 || o.alleles_cap < 0 || (n_pairs > 0 && (!a.pairs || !o.seg_of_pair)) ||
        (n_segs > 0 && (!o.segs || !o.n_found))) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_pool(who, c->aln_offs, n_segs, o.segs, n_pairs, a.pairs, o.seg_of_pair, rule.max_sites, PLAN_REFUSE_LONG)) return ioc_fail(c, st, p.msg);
    const int64_t bound = pile_sites_bound(p.segs, rule.max_sites);
    if (o.sites_cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": sites_cap " + std::to_string(o.sites_cap) + " below the bound " + std::to_string(bound));
    if ((o.out_alleles || !split) && o.alleles_cap < p.alleles_bound)
        return ioc_fail(c, IOC_ERR_CAPACITY, who + ": alleles_cap " + std::to_string(o.alleles_cap) + " below the bound " + std::to_string(p.alleles_bound));
    if ((bound > 0 && !o.out_sites) || (p.alleles_bound > 0 && !o.out_alleles && !split)) return IOC_ERR_ARG;
    if (gp) IOC_TRY(group_polish_ok(c, who, *gp, p.segs));
    for (int32_t i = 0; i < n_pairs && out_stats; ++i) out_stats[i] = ioc_aln_stats{};
    if (gp) gp->call.off[0] = 0;
    o.site_off[0] = 0;
    for (int32_t i = 0; i <= n_pairs; ++i) o.allele_off[i] = 0;
    if (n_segs == 0) return a.run(c, nullptr);
    SinkRun r{c};
    PiledDev piled;
    SitesDev sd;
    Planes laid{};  // (where each stage leaves what it made)
    IOC_TRY(r.pile(a, PileKind::counts, out_stats, p.row_base.data(), p.n_rows, p.plane.data(), p.plane_bytes, PileProject{/*ins*/ gp != nullptr}, piled));
    IOC_TRY(r.sites(rule, p, piled.cols, o.out_sites, o.site_off, o.n_found, sd));
    IOC_TRY(r.alleles(sd, p, o.seg_of_pair, piled, o.site_off, o.allele_off, o.out_alleles));
    if (split) IOC_TRY(r.split(*split, size_t(n_segs), size_t(n_pairs), o.seg_of_pair, o.site_off, o.allele_off, sd.sites, sd.alleles, true, laid));
    // The a_call hand-over: `sd` points into a_call, which the call stage of the group polish reserves again and overwrites.  The
    // split was the last to read the sites and the alleles there, and it has waited for the stream and copied out: `sd` is dead from
    // here on.  The planes are where the walks left them (a_planes), the lists and the group bytes where the split did (a_split).
    laid.base = piled.base, laid.slots = piled.slots;
    if (gp)
        IOC_TRY(group_polish_device(r, *gp, p, static_cast<const uint8_t*>(c->a_pool.p), uint64_t(c->aln_offs.back()), o.seg_of_pair,
                               Planes{nullptr, nullptr, split->out_group, nullptr, nullptr}, laid));
    IOC_TRY(r.copy_out({{o.out_cols, piled.cols, size_t(p.n_rows) * sizeof(ioc_pileup_col)}}));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: sites: %d segments, %lld rows, %lld sites kept, %lld allele bytes, %.3f MB (sites, alleles, lengths%s%s) copied from the device in %.3f ms, k_ops_pileup %.3f ms, k_ops_project %.3f ms, k_pile_sites %.3f ms, k_site_alleles %.3f ms%s\n",
                n_segs, (long long)p.n_rows, (long long)o.site_off[n_segs], (long long)o.allele_off[n_pairs], double(r.t.copied) * 1e-6, o.out_cols ? ", table" : "",
                out_stats ? ", statistics" : "", r.t.ms_copy, r.t.ms_pileup, r.t.ms_project, r.t.ms_sites, r.t.ms_alleles,
                out_stats ? (", k_ops_stats " + std::to_string(r.t.ms_stats) + " ms").c_str() : "");
    if (split && getenv("IOC_TRACE")) fprintf(stderr, "[ioc]   aligner: split: %s\n", split_trace(r.t).c_str());
    if (gp && getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: split polish: %d group-segments, %lld bytes called, k_ops_project_ins %.3f ms, k_plane_pile %.3f ms, k_pile_call %.3f ms\n",
                2 * n_segs, (long long)gp->call.off[2 * n_segs], r.t.ms_project_ins, r.t.ms_plane_pile, r.t.ms_call);
    return IOC_OK;
}

}  // namespace

int64_t ioc_align_ops_bound(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs)
{
    if (!c || n_pairs < 0 || (n_pairs > 0 && !pairs)) return IOC_ERR_ARG;
    int64_t bound = 0;
    for (int32_t i = 0; i < n_pairs; ++i) {
        IOC_TRY(ioc_pair_in_pool(c, pairs[i]));
        bound += ioc_seq_len(c, pairs[i].query) + ioc_seq_len(c, pairs[i].ref);
    }
    return bound;
}

// The walks write a pair's bytes into a region of its own of the caller's buffer (as long as the pair's share of the bound);
// the regions are packed when all runs — the call's own, the re-runs' — are over.
int ioc_align_pairs_ops(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                        int32_t* out_score, int64_t* out_windows, double* out_ratio, char* out_ops, int64_t ops_cap, int64_t* ops_off)
{
    if (!c || n_pairs < 0 || (n_pairs > 0 && !pairs) || !ops_off || ops_cap < 0 || (ops_cap > 0 && !out_ops)) return IOC_ERR_ARG;
    const int64_t bound = ioc_align_ops_bound(c, n_pairs, pairs);
    if (bound < 0) return int(bound);
    if (ops_cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, "ioc_align_pairs_ops: ops_cap " + std::to_string(ops_cap) + " below the bound " + std::to_string(bound));
    std::vector<int64_t> base(size_t(n_pairs) + 1, 0), len(size_t(n_pairs), 0);
    for (int32_t i = 0; i < n_pairs; ++i) base[size_t(i) + 1] = base[size_t(i)] + ioc_seq_len(c, pairs[i].query) + ioc_seq_len(c, pairs[i].ref);
    AlnTally t;
    const AlnSink sink{SinkKind::bytes, len.data(), &t, {reinterpret_cast<uint8_t*>(out_ops), base.data()}};
    IOC_TRY((AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}.run(c, &sink)));
    ops_off[0] = 0;
    for (int32_t i = 0; i < n_pairs; ++i) {  // (a packed position never lies behind the region's own)
        if (len[size_t(i)] > 0 && ops_off[i] != base[size_t(i)]) memmove(out_ops + ops_off[i], out_ops + base[size_t(i)], size_t(len[size_t(i)]));
        ops_off[i + 1] = ops_off[i] + len[size_t(i)];
    }
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: operation bytes: %.1f MB copied from the device in %.3f ms, %.1f MB packed\n", double(t.copied) * 1e-6, t.ms_copy,
                double(ops_off[n_pairs]) * 1e-6);
    return IOC_OK;
}

// The walks write a slice's bytes as for ioc_align_pairs_ops; k_ops_stats (ioc_ops_stats.hip) reduces them where they lie, and
// the records of the run that counted — the call's own, a re-run's — end up in out_stats.
int ioc_align_pairs_stats(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                          int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats)
{
    if (!c || n_pairs < 0 || (n_pairs > 0 && (!pairs || !out_stats))) return IOC_ERR_ARG;
    for (int32_t i = 0; i < n_pairs && out_stats; ++i) out_stats[i] = ioc_aln_stats{};
    std::vector<int64_t> len(size_t(n_pairs), 0);
    AlnTally t;
    const AlnSink sink{SinkKind::reduced, len.data(), &t, {}, true, out_stats};
    IOC_TRY((AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}.run(c, &sink)));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: alignment statistics: %lld records (%.3f MB with the lengths) copied from the device in %.3f ms, k_ops_stats %.3f ms\n",
                (long long)t.records, double(t.copied) * 1e-6, t.ms_copy, t.ms_stats);
    return IOC_OK;
}

// pile -> copy-out.  The walks write a slice's bytes as for ioc_align_pairs_ops; k_ops_pileup (ioc_ops_pileup.hip) adds them,
// where they lie, into a table of the call's rows that stays on the device over the slices and the re-runs and is copied out once.
int ioc_align_pairs_pileup(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                           int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, const int64_t* row_base, int64_t
                           n_rows, ioc_pileup_col* out_cols)
{
    if (!c || n_pairs < 0 || n_rows < 0 || (n_pairs > 0 && (!pairs || !row_base || !out_cols))) return IOC_ERR_ARG;
    for (int32_t i = 0; i < n_pairs; ++i) {
        IOC_TRY(ioc_pair_in_pool(c, pairs[i]));
        if (row_base[i] < 0 || row_base[i] > n_rows - ioc_seq_len(c, pairs[i].ref) - 1)
            return ioc_fail(c, IOC_ERR_ARG, "ioc_align_pairs_pileup: the rows of pair " + std::to_string(i) + " lie outside the table");
    }
    for (int32_t i = 0; i < n_pairs && out_stats; ++i) out_stats[i] = ioc_aln_stats{};
    if (out_cols && n_rows > 0) memset(out_cols, 0, size_t(n_rows) * sizeof(ioc_pileup_col));
    const AlnCall a{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio};
    if (n_pairs == 0 || n_rows == 0) return a.run(c, nullptr);
    SinkRun r{c};
    PiledDev d;
    IOC_TRY(r.pile(a, PileKind::counts, out_stats, row_base, n_rows, nullptr, 0, PileProject{}, d));
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    IOC_TRY(r.copy_out({{out_cols, d.cols, size_t(n_rows) * sizeof(ioc_pileup_col)}}));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: pileup: %lld rows, %.3f MB (table, lengths%s) copied from the device in %.3f ms, k_ops_pileup %.3f ms%s\n",
                (long long)n_rows, double(r.t.copied) * 1e-6, out_stats ? ", statistics" : "", r.t.ms_copy, r.t.ms_pileup,
                out_stats ? (", k_ops_stats " + std::to_string(r.t.ms_stats) + " ms").c_str() : "");
    return IOC_OK;
}

// upload -> sites
int ioc_pileup_sites(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const ioc_pileup_col* cols, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                     int32_t max_sites, ioc_pile_site* out_sites, int64_t sites_cap, int64_t* site_off, int64_t* n_found)
{
    const SitesRule rule{min_depth, min_alt, min_pct, max_sites};
    if (!c || n_segs < 0 || !rule.ok() || !site_off || sites_cap < 0 || (n_segs > 0 && (!rlen || !cols || !n_found))) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen("ioc_pileup_sites", n_segs, rlen, nullptr, nullptr, 0, nullptr, nullptr, PLAN_REFUSE_LONG)) return ioc_fail(c, st, p.msg);
    const int64_t bound = pile_sites_bound(p.segs, max_sites);
    if (sites_cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, "ioc_pileup_sites: sites_cap " + std::to_string(sites_cap) + " below the bound " + std::to_string(bound));
    if (bound > 0 && !out_sites) return IOC_ERR_ARG;
    site_off[0] = 0;
    if (n_segs == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    const size_t b_cols = size_t(p.n_rows) * sizeof(ioc_pileup_col);
    IOC_TRY(ioc_reserve(c, c->a_pile, b_cols));
    IOC_CHK(c, hipMemcpyAsync(c->a_pile.p, cols, b_cols, hipMemcpyHostToDevice, c->stream));
    SinkRun r{c};
    SitesDev sd;
    IOC_TRY(r.sites(rule, p, c->a_pile.as<ioc_pileup_col>(), out_sites, site_off, n_found, sd));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   site search: %d segments, %lld rows, %lld sites kept, k_pile_sites %.3f ms\n", n_segs, (long long)p.n_rows,
                (long long)site_off[n_segs], r.t.ms_sites);
    return IOC_OK;
}

int ioc_align_pairs_alleles(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                            int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                            const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites,
                            ioc_pile_site* out_sites, int64_t sites_cap, int64_t* site_off, int64_t* n_found, uint8_t* out_alleles, int64_t alleles_cap,
                            int64_t* allele_off, ioc_pileup_col* out_cols)
{
    return align_pairs_alleles("ioc_align_pairs_alleles", c, AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats,
                               SitesRule{min_depth, min_alt, min_pct, max_sites}, AllelesCall{n_segs, segs, seg_of_pair, out_sites, out_alleles, out_cols,
                               sites_cap, alleles_cap, site_off, n_found, allele_off}, nullptr, nullptr);
}

// ioc_align_pairs_alleles with the split kernels (ioc_site_split.hip) run over the sites and the alleles where k_pile_sites and
// k_site_alleles left them: one byte per read comes back, and the alleles only where they are asked for.
int ioc_align_pairs_split(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                          int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                          const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites,
                          ioc_pile_site* out_sites, int64_t sites_cap, int64_t* site_off, int64_t* n_found, uint8_t* out_alleles, int64_t alleles_cap,
                          int64_t* allele_off, ioc_pileup_col* out_cols, int32_t min_link, int32_t min_margin, int32_t rounds, int64_t* out_link,
                          int8_t* out_phase, uint8_t* out_group, int32_t* out_vote, ioc_split_seg* out_seg)
{
    const SplitCall sp{min_link, min_margin, rounds, out_link, out_phase, out_group, out_vote, out_seg};
    return align_pairs_alleles("ioc_align_pairs_split", c, AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats,
                               SitesRule{min_depth, min_alt, min_pct, max_sites}, AllelesCall{n_segs, segs, seg_of_pair, out_sites, out_alleles, out_cols,
                               sites_cap, alleles_cap, site_off, n_found, allele_off}, &sp, nullptr);
}

// ioc_align_pairs_split with the six slot planes projected beside the two, and behind k_split_record k_plane_pile and the call
// kernels over the planes: the consensus of both groups of every segment, with no pair aligned a second time.
int ioc_align_pairs_split_polish(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                 int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                 const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                                 int32_t max_sites, ioc_pile_site* out_sites, int64_t sites_cap, int64_t* site_off, int64_t* n_found, uint8_t* out_alleles,
                                 int64_t alleles_cap, int64_t* allele_off, ioc_pileup_col* out_cols, int32_t min_link, int32_t min_margin, int32_t rounds,
                                 int64_t* out_link, int8_t* out_phase, uint8_t* out_group, int32_t* out_vote, ioc_split_seg* out_seg,
                                 int32_t polish_min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish,
                                 ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins)
{
    const SplitCall sp{min_link, min_margin, rounds, out_link, out_phase, out_group, out_vote, out_seg};
    const GroupPolish gp{{polish_min_depth, out_seq, out_qual, cap, out_off, out_polish}, out_gcols, out_gins};
    return align_pairs_alleles("ioc_align_pairs_split_polish", c, AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio},
                               out_stats, SitesRule{min_depth, min_alt, min_pct, max_sites}, AllelesCall{n_segs, segs, seg_of_pair, out_sites, out_alleles, out_cols,
                               sites_cap, alleles_cap, site_off, n_found, allele_off}, &sp, &gp);
}

// upload -> group pile -> call -> copy-out.  The group polish from planes the caller holds: everything is uploaded, and the
// kernels run as behind ioc_align_pairs_split_polish.
int ioc_planes_polish(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, int32_t n_pairs,
                      const int32_t* seg_of_pair, const uint8_t* group, const uint8_t* base, const uint8_t* slots, int32_t min_depth, char* out_seq,
                      char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish, ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins)
{
    const GroupPolish gp{{min_depth, out_seq, out_qual, cap, out_off, out_polish}, out_gcols, out_gins};
    if (!c || n_segs < 0 || n_pairs < 0 || !gp.call.ok() || (n_segs > 0 && (!rlen || !frame_off)) || (n_pairs > 0 && (!seg_of_pair || !group))) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen("ioc_planes_polish", n_segs, rlen, frames, frame_off, n_pairs, seg_of_pair, group, 0)) return ioc_fail(c, st, p.msg);
    if (p.plane_bytes > 0 && (!base || !slots)) return IOC_ERR_ARG;
    IOC_TRY(group_polish_ok(c, "ioc_planes_polish", gp, p.segs));
    out_off[0] = 0;
    if (n_segs == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    DevBuf d_frames;
    IOC_TRY(ioc_alloc(c, d_frames, size_t(p.frame_bytes)));
    if (p.frame_bytes > 0) IOC_CHK(c, hipMemcpyAsync(d_frames.p, frames, size_t(p.frame_bytes), hipMemcpyHostToDevice, c->stream));
    SinkRun r{c};
    IOC_TRY(group_polish_device(r, gp, p, static_cast<const uint8_t*>(d_frames.p), uint64_t(p.frame_bytes), seg_of_pair, Planes{nullptr, nullptr, group, base, slots}, Planes{}));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes polish: %d group-segments, %lld rows, %d pairs, %lld plane bytes, %lld bytes called, k_plane_pile %.3f ms, k_pile_call %.3f ms\n",
                2 * n_segs, (long long)(2 * p.n_rows), n_pairs, (long long)(8 * p.plane_bytes), (long long)out_off[2 * n_segs], r.t.ms_plane_pile, r.t.ms_call);
    return IOC_OK;
}

// what a call over n_groups[g] groups of segment g refuses once its segments are known, and what it may call: the bound is the sum
// over the segments of n_groups[g] * pile_call_most(rlen[g])
static int groups_polish_ok(ioc_ctx* c, const std::string& who, const CallOut& o, const std::vector<IocPileSeg>& ds, const int32_t* n_groups)
{
    int64_t bound = 0;
    for (size_t g = 0; g < ds.size(); ++g) {
        if (pile_call_most(ds[g].rlen) > INT32_MAX)  // (the record's out_len, the kernels' byte counts)
            return ioc_fail(c, IOC_ERR_CAPACITY, who + ": segment " + std::to_string(g) + " may call more than 2^31 - 1 bytes");
        bound += int64_t(n_groups[g]) * pile_call_most(ds[g].rlen);
    }
    return call_room_ok(c, who, o, bound);
}

// groups pile -> call -> copy-out: the consensus of every group of every segment (frames in d_frames), the group tables where asked for
static int groups_polish_device(SinkRun& r, const GroupPolish& gp, const SinkPlan& p, const uint8_t* d_frames, uint64_t frame_bytes, const int32_t* seg_of_pair,
                                const int32_t* group, const int32_t* n_groups, const Planes& host, const Planes& dev)
{
    GroupPiled g;
    IOC_TRY(r.groups_pile(p, seg_of_pair, group, n_groups, host, dev, g));
    IOC_TRY(pile_call_device(r, g.gsegs, d_frames, frame_bytes, gp.call, g.cols, g.ins, nullptr, g.n_rows));
    return r.copy_out({{gp.out_gcols, g.cols, size_t(g.n_rows) * sizeof(ioc_pileup_col)}, {gp.out_gins, g.ins, size_t(g.n_rows) * sizeof(ioc_pileup_ins)}});
}

// weighted groups pile -> weighted call -> copy-out: the weighted consensus of every group of every segment (frames in d_frames) —
// the counts gate, the sums of weights decide (pile_call_device with d_gate) —, the three group tables where asked for
struct GroupTablesW {
    ioc_pileup_col *out_gcols, *out_gwcols;
    ioc_pileup_ins* out_gwins;
};
static int groups_polish_weighted_device(SinkRun& r, const CallOut& call, const GroupTablesW& o, const SinkPlan& p, const uint8_t* d_frames, uint64_t frame_bytes,
                                         const int32_t* seg_of_pair, const int32_t* group, const int32_t* n_groups, const Planes& host, const Planes& dev)
{
    GroupPiled g;
    IOC_TRY(r.groups_pile(p, seg_of_pair, group, n_groups, host, dev, g, /*weighted*/ true));
    IOC_TRY(pile_call_device(r, g.gsegs, d_frames, frame_bytes, call, g.wcols, g.wins, g.cols, g.n_rows));
    const size_t b_cols = size_t(g.n_rows) * sizeof(ioc_pileup_col);
    return r.copy_out({{o.out_gcols, g.cols, b_cols}, {o.out_gwcols, g.wcols, b_cols}, {o.out_gwins, g.wins, size_t(g.n_rows) * sizeof(ioc_pileup_ins)}});
}

// upload -> groups pile -> call -> copy-out.  ioc_planes_polish over any number of groups a segment: everything is uploaded, every
// group's own member list with it, and k_group_pile and the call kernels run as behind ioc_align_pairs_blocks_polish.
int ioc_planes_polish_groups(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, const int32_t* n_groups,
                             int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* group, const uint8_t* base, const uint8_t* slots, int32_t min_depth,
                             char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish, ioc_pileup_col* out_gcols,
                             ioc_pileup_ins* out_gins)
{
    const std::string who = "ioc_planes_polish_groups";
    const GroupPolish gp{{min_depth, out_seq, out_qual, cap, out_off, out_polish}, out_gcols, out_gins};
    if (!c || n_segs < 0 || n_pairs < 0 || !gp.call.ok() || (n_segs > 0 && (!rlen || !frame_off || !n_groups)) || (n_pairs > 0 && (!seg_of_pair || !group)))
        return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen(who, n_segs, rlen, frames, frame_off, n_pairs, seg_of_pair, nullptr, 0)) return ioc_fail(c, st, p.msg);
    if (p.plane_bytes > 0 && (!base || !slots)) return IOC_ERR_ARG;
    int64_t G = 0;
    for (int32_t g = 0; g < n_segs; ++g) {
        if (n_groups[g] < 0) return ioc_fail(c, IOC_ERR_ARG, who + ": segment " + std::to_string(g) + " has a negative number of groups");
        if ((G += n_groups[g]) > INT32_MAX) return ioc_fail(c, IOC_ERR_ARG, who + ": more than 2^31 - 1 group-segments");
    }
    for (int32_t i = 0; i < n_pairs; ++i)
        if (group[i] < -1 || group[i] >= n_groups[seg_of_pair[i]])
            return ioc_fail(c, IOC_ERR_ARG, who + ": the group of pair " + std::to_string(i) + " is neither -1 nor one of its segment's");
    IOC_TRY(groups_polish_ok(c, who, gp.call, p.segs, n_groups));
    out_off[0] = 0;
    if (G == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    DevBuf d_frames;
    IOC_TRY(ioc_alloc(c, d_frames, size_t(p.frame_bytes)));
    if (p.frame_bytes > 0) IOC_CHK(c, hipMemcpyAsync(d_frames.p, frames, size_t(p.frame_bytes), hipMemcpyHostToDevice, c->stream));
    SinkRun r{c};
    IOC_TRY(groups_polish_device(r, gp, p, static_cast<const uint8_t*>(d_frames.p), uint64_t(p.frame_bytes), seg_of_pair, group, n_groups,
                                 Planes{nullptr, nullptr, nullptr, base, slots}, Planes{}));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes polish groups: %lld group-segments, %d pairs, %lld plane bytes, %lld bytes called, k_group_pile %.3f ms, k_pile_call %.3f ms\n",
                (long long)G, n_pairs, (long long)(7 * p.plane_bytes), (long long)out_off[G], r.t.ms_group_pile, r.t.ms_call);
    return IOC_OK;
}

// upload -> weighted groups pile -> weighted call -> copy-out.  ioc_planes_polish_groups with every read's vote counted by its
// weight: the seven weight planes are uploaded beside the seven, k_group_pile_weighted adds up the three tables of every group and
// the weighted mode of the call kernels runs over the group-segments.  The checks of ioc_planes_polish_groups, in its order.
int ioc_planes_polish_groups_weighted(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, const int32_t* n_groups,
                                      int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* group, const uint8_t* base, const uint8_t* slots,
                                      const uint8_t* wbase, const uint8_t* wslots, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off,
                                      ioc_polish_stats* out_polish, ioc_pileup_col* out_gcols, ioc_pileup_col* out_gwcols, ioc_pileup_ins* out_gwins)
{
    const std::string who = "ioc_planes_polish_groups_weighted";
    const CallOut call{min_depth, out_seq, out_qual, cap, out_off, out_polish};
    if (!c || n_segs < 0 || n_pairs < 0 || !call.ok() || (n_segs > 0 && (!rlen || !frame_off || !n_groups)) || (n_pairs > 0 && (!seg_of_pair || !group)))
        return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen(who, n_segs, rlen, frames, frame_off, n_pairs, seg_of_pair, nullptr, 0)) return ioc_fail(c, st, p.msg);
    if (p.plane_bytes > 0 && (!base || !slots)) return IOC_ERR_ARG;
    if (n_pairs > 0 && (!wbase || !wslots)) return IOC_ERR_ARG;
    int64_t G = 0;
    for (int32_t g = 0; g < n_segs; ++g) {
        if (n_groups[g] < 0) return ioc_fail(c, IOC_ERR_ARG, who + ": segment " + std::to_string(g) + " has a negative number of groups");
        if ((G += n_groups[g]) > INT32_MAX) return ioc_fail(c, IOC_ERR_ARG, who + ": more than 2^31 - 1 group-segments");
    }
    for (int32_t i = 0; i < n_pairs; ++i)
        if (group[i] < -1 || group[i] >= n_groups[seg_of_pair[i]])
            return ioc_fail(c, IOC_ERR_ARG, who + ": the group of pair " + std::to_string(i) + " is neither -1 nor one of its segment's");
    IOC_TRY(groups_polish_ok(c, who, call, p.segs, n_groups));
    out_off[0] = 0;
    if (G == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    DevBuf d_frames;
    IOC_TRY(ioc_alloc(c, d_frames, size_t(p.frame_bytes)));
    if (p.frame_bytes > 0) IOC_CHK(c, hipMemcpyAsync(d_frames.p, frames, size_t(p.frame_bytes), hipMemcpyHostToDevice, c->stream));
    SinkRun r{c};
    Planes host{nullptr, nullptr, nullptr, base, slots};
    host.wbase = wbase, host.wslots = wslots;
    IOC_TRY(groups_polish_weighted_device(r, call, GroupTablesW{out_gcols, out_gwcols, out_gwins}, p, static_cast<const uint8_t*>(d_frames.p),
                                          uint64_t(p.frame_bytes), seg_of_pair, group, n_groups, host, Planes{}));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes polish groups weighted: %lld group-segments, %d pairs, %lld plane bytes, %lld bytes called, k_group_pile_weighted %.3f ms, k_pile_call<weighted> %.3f ms\n",
                (long long)G, n_pairs, (long long)(14 * p.plane_bytes), (long long)out_off[G], r.t.ms_group_pile_weighted, r.t.ms_call);
    return IOC_OK;
}

// what a read correction refuses once its plan is known: IOC_OK, or the status with the message set
static int correct_room_ok(ioc_ctx* c, const std::string& who, const CorrectOut& o, const SinkPlan& p)
{
    for (size_t g = 0; g < p.segs.size(); ++g)
        if (pile_call_most(p.segs[g].rlen) > INT32_MAX)  // (the record's out_len, the kernels' byte counts)
            return ioc_fail(c, IOC_ERR_CAPACITY, who + ": segment " + std::to_string(g) + " may call more than 2^31 - 1 bytes");
    if (o.cap < p.correct_bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": cap " + std::to_string(o.cap) + " below the bound " + std::to_string(p.correct_bound));
    return p.correct_bound > 0 && (!o.seq || !o.qual) ? IOC_ERR_ARG : IOC_OK;
}

// upload -> correct -> copy-out.  The read correction from planes and tables the caller holds: everything is uploaded, and the
// kernels run as behind ioc_align_pairs_correct.
int ioc_planes_correct(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, const ioc_pileup_col* cols,
                       const ioc_pileup_ins* ins, int32_t n_pairs, const int32_t* seg_of_pair, const uint8_t* base, const uint8_t* slots, int32_t min_depth,
                       int32_t min_alt, int32_t min_pct, int32_t max_run, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_correct_stats* out_stats)
{
    const CorrectOut o{{min_depth, min_alt, min_pct, max_run}, out_seq, out_qual, cap, out_off, out_stats};
    if (!c || n_segs < 0 || n_pairs < 0 || !o.ok() || (n_segs > 0 && (!rlen || !frame_off || !cols || !ins)) || (n_pairs > 0 && !seg_of_pair)) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen("ioc_planes_correct", n_segs, rlen, frames, frame_off, n_pairs, seg_of_pair, nullptr, PLAN_REFUSE_CALLED)) return ioc_fail(c, st, p.msg);
    if (p.plane_bytes > 0 && (!base || !slots)) return IOC_ERR_ARG;
    IOC_TRY(correct_room_ok(c, "ioc_planes_correct", o, p));
    out_off[0] = 0;
    if (n_pairs == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    const size_t b_cols = size_t(p.n_rows) * sizeof(ioc_pileup_col), b_ins = size_t(p.n_rows) * sizeof(ioc_pileup_ins);
    IOC_TRY(ioc_reserve(c, c->a_pile, b_cols));
    IOC_TRY(ioc_reserve(c, c->a_pile_ins, b_ins));
    DevBuf d_frames;
    IOC_TRY(ioc_alloc(c, d_frames, size_t(p.frame_bytes)));
    IOC_CHK(c, hipMemcpyAsync(c->a_pile.p, cols, b_cols, hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemcpyAsync(c->a_pile_ins.p, ins, b_ins, hipMemcpyHostToDevice, c->stream));
    if (p.frame_bytes > 0) IOC_CHK(c, hipMemcpyAsync(d_frames.p, frames, size_t(p.frame_bytes), hipMemcpyHostToDevice, c->stream));
    SinkRun r{c};
    IOC_TRY(r.correct(p, seg_of_pair, static_cast<const uint8_t*>(d_frames.p), uint64_t(p.frame_bytes), c->a_pile.as<ioc_pileup_col>(), c->a_pile_ins.as<ioc_pileup_ins>(),
                      Planes{nullptr, nullptr, nullptr, base, slots}, Planes{}, o));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes correct: %d segments, %lld rows, %d pairs, %lld plane bytes, %lld bytes written, k_read_correct %.3f ms\n", n_segs,
                (long long)p.n_rows, n_pairs, (long long)(7 * p.plane_bytes), (long long)out_off[n_pairs], r.t.ms_correct);
    return IOC_OK;
}

// what a read correction by isoform refuses once its plan and its reads are known: IOC_OK, or the status with the message set.
// The bound is the sum over the pairs of their segment's call bound and their read's length; a pair's own share fits 31 bits (the
// record's out_len, the kernels' byte counts).
static int iso_correct_room_ok(ioc_ctx* c, const std::string& who, const IsoCorrectOut& o, const SinkPlan& p, const int32_t* seg_of_pair, const std::vector<uint32_t>& q_len)
{
    int64_t bound = p.correct_bound;
    for (size_t i = 0; i < q_len.size(); ++i) {
        if (pile_call_most(p.segs[size_t(seg_of_pair[i])].rlen) + int64_t(q_len[i]) > INT32_MAX)
            return ioc_fail(c, IOC_ERR_CAPACITY, who + ": pair " + std::to_string(i) + " may write more than 2^31 - 1 bytes");
        bound += q_len[i];
    }
    if (o.cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": cap " + std::to_string(o.cap) + " below the bound " + std::to_string(bound));
    return bound > 0 && (!o.seq || !o.qual) ? IOC_ERR_ARG : IOC_OK;
}

// upload -> groups pile -> iso correct -> copy-out.  The read correction by isoform from planes the caller holds, over the pool that
// is set: everything is uploaded, and the kernels run as behind ioc_align_pairs_blocks_correct.  The checks of ioc_planes_correct and
// of ioc_planes_polish_groups, in their order, then the queries.
int ioc_planes_correct_groups(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, const int32_t* n_groups, int32_t n_pairs,
                              const int32_t* seg_of_pair, const int32_t* group, const int32_t* query, const uint8_t* base, const uint8_t* slots, const uint8_t* ilen,
                              const uint32_t* qpos, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run, char* out_seq, char* out_qual, int64_t cap,
                              int64_t* out_off, ioc_iso_correct_stats* out_stats)
{
    const std::string who = "ioc_planes_correct_groups";
    const IsoCorrectOut o{{min_depth, min_alt, min_pct, max_run}, out_seq, out_qual, cap, out_off, out_stats};
    if (!c || n_segs < 0 || n_pairs < 0 || !o.ok() || (n_segs > 0 && (!rlen || !frame_off || !n_groups)) || (n_pairs > 0 && (!seg_of_pair || !group || !query)))
        return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen(who, n_segs, rlen, frames, frame_off, n_pairs, seg_of_pair, nullptr, PLAN_REFUSE_CALLED)) return ioc_fail(c, st, p.msg);
    if (p.plane_bytes > 0 && (!base || !slots || !ilen || !qpos)) return IOC_ERR_ARG;
    int64_t G = 0;
    for (int32_t g = 0; g < n_segs; ++g) {
        if (n_groups[g] < 0) return ioc_fail(c, IOC_ERR_ARG, who + ": segment " + std::to_string(g) + " has a negative number of groups");
        if ((G += n_groups[g]) + n_segs > INT32_MAX) return ioc_fail(c, IOC_ERR_ARG, who + ": more than 2^31 - 1 group-segments");
    }
    std::vector<uint64_t> q_off(size_t(n_pairs), 0);
    std::vector<uint32_t> q_len(size_t(n_pairs), 0);
    for (int32_t i = 0; i < n_pairs; ++i) {
        if (group[i] < -1 || group[i] >= n_groups[seg_of_pair[i]])
            return ioc_fail(c, IOC_ERR_ARG, who + ": the group of pair " + std::to_string(i) + " is neither -1 nor one of its segment's");
        if (query[i] < 0 || size_t(query[i]) + 1 >= c->aln_offs.size()) return ioc_fail(c, IOC_ERR_ARG, who + ": the read of pair " + std::to_string(i) + " lies outside the pool");
        q_off[size_t(i)] = uint64_t(c->aln_offs[size_t(query[i])]), q_len[size_t(i)] = uint32_t(ioc_seq_len(c, query[i]));
    }
    IOC_TRY(iso_correct_room_ok(c, who, o, p, seg_of_pair, q_len));
    out_off[0] = 0;
    if (n_pairs == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    DevBuf d_frames;
    IOC_TRY(ioc_alloc(c, d_frames, size_t(p.frame_bytes)));
    if (p.frame_bytes > 0) IOC_CHK(c, hipMemcpyAsync(d_frames.p, frames, size_t(p.frame_bytes), hipMemcpyHostToDevice, c->stream));
    SinkRun r{c};
    IOC_TRY(r.iso_correct(p, seg_of_pair, group, n_groups, static_cast<const uint8_t*>(d_frames.p), uint64_t(p.frame_bytes), Planes{nullptr, nullptr, nullptr, base, slots},
                          Planes{}, LongPlanes{ilen, qpos}, LongPlanes{}, q_off, q_len, o));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes correct groups: %d segments, %lld group-segments and %d of all pairs, %d pairs, %lld plane bytes, %lld bytes written, k_group_pile %.3f ms, k_iso_correct %.3f ms\n",
                n_segs, (long long)G, n_segs, n_pairs, (long long)(12 * p.plane_bytes), (long long)out_off[n_pairs], r.t.ms_group_pile, r.t.ms_iso_correct);
    return IOC_OK;
}

// pile -> correct -> copy-out.  ioc_align_pairs_polish's pile with every pair projected beside it, base plane and slot planes, and
// k_read_correct over the tables and the planes where they lie: what comes back is every pair's corrected bytes and its record,
// and the tables only where they are asked for.
int ioc_align_pairs_correct(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                            int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs,
                            const int32_t* seg_of_pair, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run, char* out_seq, char* out_qual,
                            int64_t cap, int64_t* out_off, ioc_correct_stats* out_correct, ioc_pileup_col* out_cols, ioc_pileup_ins* out_ins)
{
    const AlnCall a{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio};
    const CorrectOut o{{min_depth, min_alt, min_pct, max_run}, out_seq, out_qual, cap, out_off, out_correct};
    if (!c || n_pairs < 0 || n_segs < 0 || !o.ok() || (n_pairs > 0 && (!pairs || !seg_of_pair)) || (n_segs > 0 && !segs)) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_pool("ioc_align_pairs_correct", c->aln_offs, n_segs, segs, n_pairs, pairs, seg_of_pair, 0, 0)) return ioc_fail(c, st, p.msg);
    IOC_TRY(correct_room_ok(c, "ioc_align_pairs_correct", o, p));
    for (int32_t i = 0; i < n_pairs && out_stats; ++i) out_stats[i] = ioc_aln_stats{};
    out_off[0] = 0;
    if (n_segs == 0) return a.run(c, nullptr);
    SinkRun r{c};
    PiledDev d;
    IOC_TRY(r.pile(a, PileKind::ins, out_stats, p.row_base.data(), p.n_rows, p.plane.data(), p.plane_bytes, PileProject{/*ins*/ true}, d));
    IOC_TRY(r.correct(p, seg_of_pair, static_cast<const uint8_t*>(c->a_pool.p), uint64_t(c->aln_offs.back()), d.cols, d.ins, Planes{},
                      Planes{nullptr, nullptr, nullptr, d.base, d.slots}, o));
    IOC_CHK(c, hipStreamSynchronize(c->stream));  // (a call without pairs has launched nothing that waited)
    IOC_TRY(r.copy_out({{out_cols, d.cols, size_t(p.n_rows) * sizeof(ioc_pileup_col)}, {out_ins, d.ins, size_t(p.n_rows) * sizeof(ioc_pileup_ins)}}));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: correct: %d segments, %lld rows, %d pairs, %lld bytes written, %.3f MB (corrected bytes, records, lengths%s%s) copied from the device in %.3f ms, k_ops_pileup<ins> %.3f ms, k_ops_project %.3f ms, k_ops_project_ins %.3f ms, k_read_correct %.3f ms%s\n",
                n_segs, (long long)p.n_rows, n_pairs, (long long)out_off[n_pairs], double(r.t.copied) * 1e-6, out_cols || out_ins ? ", tables" : "",
                out_stats ? ", statistics" : "", r.t.ms_copy, r.t.ms_pileup, r.t.ms_project, r.t.ms_project_ins, r.t.ms_correct,
                out_stats ? (", k_ops_stats " + std::to_string(r.t.ms_stats) + " ms").c_str() : "");
    return IOC_OK;
}

// what a block search refuses once its plan is known: IOC_OK, or the status with the message set
static int blocks_room_ok(ioc_ctx* c, const std::string& who, const BlocksOut& o, const SinkPlan& p)
{
    const int64_t bound = p.blocks_bound(o.rule.max_blocks);
    if (o.cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": blocks_cap " + std::to_string(o.cap) + " below the bound " + std::to_string(bound));
    return (bound > 0 && !o.blocks) || (!p.plane.empty() && !o.reads) || (!p.segs.empty() && !o.seg) ? IOC_ERR_ARG : IOC_OK;
}

// upload -> blocks -> copy-out.  The block search from base planes the caller holds: they are uploaded, and the kernels run as
// behind ioc_align_pairs_blocks.
int ioc_planes_blocks(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, int32_t n_pairs, const int32_t* seg_of_pair, const uint8_t* base, int32_t min_gap,
                      int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows,
                      ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg)
{
    const BlocksOut o{{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg};
    if (!c || n_segs < 0 || n_pairs < 0 || !o.ok() || (n_segs > 0 && !rlen) || (n_pairs > 0 && !seg_of_pair)) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen("ioc_planes_blocks", n_segs, rlen, nullptr, nullptr, n_pairs, seg_of_pair, nullptr, 0)) return ioc_fail(c, st, p.msg);
    if (p.plane_bytes > 0 && !base) return IOC_ERR_ARG;
    IOC_TRY(blocks_room_ok(c, "ioc_planes_blocks", o, p));
    block_off[0] = 0;
    if (n_segs == 0) return IOC_OK;
    SinkRun r{c};
    IOC_TRY(r.blocks(p, seg_of_pair, base, nullptr, o));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes blocks: %d segments, %lld rows, %d pairs, %lld plane bytes, %lld blocks kept, the block kernels %.3f ms\n", n_segs,
                (long long)p.n_rows, n_pairs, (long long)p.plane_bytes, (long long)block_off[n_segs], r.t.ms_blocks);
    return IOC_OK;
}

// what a search for insertion sites refuses once its plan is known: IOC_OK, or the status with the message set
static int64_t inserts_bound(const SinkPlan& p, int32_t max_sites)
{
    int64_t b = 0;
    for (const IocPileSeg& sg : p.segs) b += inserts_sites_most(sg.rlen, max_sites);
    return b;
}
static int inserts_room_ok(ioc_ctx* c, const std::string& who, const InsertsOut& o, const SinkPlan& p)
{
    const int64_t bound = inserts_bound(p, o.rule.max_sites);
    if (o.cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": sites_cap " + std::to_string(o.cap) + " below the bound " + std::to_string(bound));
    return (bound > 0 && !o.sites) || (!p.plane.empty() && !o.reads) || (!p.segs.empty() && !o.seg) ? IOC_ERR_ARG : IOC_OK;
}
static std::string inserts_trace(const AlnTally& t)
{
    char buf[400];
    snprintf(buf, sizeof buf, "k_ins_bits %.3f ms, k_ins_rows %.3f ms, k_ins_list %.3f ms, k_ins_states %.3f ms, k_ins_lens %.3f ms, k_ins_support %.3f ms, k_ins_isoforms %.3f ms, k_ins_record %.3f ms",
             t.ms_inserts[0], t.ms_inserts[1], t.ms_inserts[2], t.ms_inserts[3], t.ms_inserts[4], t.ms_inserts[5], t.ms_inserts[6], t.ms_inserts[7]);
    return buf;
}

// upload -> inserts -> copy-out.  The search for insertion sites from planes the caller holds: they are uploaded, and the kernels run
// as behind ioc_align_pairs_blocks_inserts.
int ioc_planes_inserts(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, int32_t n_pairs, const int32_t* seg_of_pair, const uint8_t* base, const uint8_t* ilen,
                       int32_t min_ins, int32_t slack, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites, const uint64_t* pre_key,
                       const uint64_t* pre_mask, const uint64_t* pre_full, ioc_insert_row* out_rows, ioc_pile_insert* out_sites, int64_t sites_cap,
                       int64_t* site_off, ioc_read_inserts* out_reads, ioc_inserts_seg* out_seg)
{
    const InsertsOut o{{min_ins, slack, min_depth, min_alt, min_pct, max_sites}, out_rows, out_sites, sites_cap, site_off, out_reads, out_seg};
    if (!c || n_segs < 0 || n_pairs < 0 || !o.ok() || (n_segs > 0 && !rlen) || (n_pairs > 0 && !seg_of_pair)) return IOC_ERR_ARG;
    const int given = (pre_key != nullptr) + (pre_mask != nullptr) + (pre_full != nullptr);
    if (given != 0 && given != 3) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen("ioc_planes_inserts", n_segs, rlen, nullptr, nullptr, n_pairs, seg_of_pair, nullptr, 0)) return ioc_fail(c, st, p.msg);
    if (p.plane_bytes > 0 && (!base || !ilen)) return IOC_ERR_ARG;
    IOC_TRY(inserts_room_ok(c, "ioc_planes_inserts", o, p));
    site_off[0] = 0;
    if (n_segs == 0) return IOC_OK;
    SinkRun r{c};
    InsertsPre pre;
    if (given && n_pairs > 0) pre.host_key = pre_key, pre.host_mask = pre_mask, pre.pre_full = pre_full;
    IOC_TRY(r.inserts(p, seg_of_pair, base, ilen, nullptr, nullptr, pre, o));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes inserts: %d segments, %lld rows, %d pairs, %lld plane bytes, %lld sites kept, %s\n", n_segs, (long long)p.n_rows, n_pairs,
                (long long)p.plane_bytes, (long long)site_off[n_segs], inserts_trace(r.t).c_str());
    return IOC_OK;
}

// what a search for ends refuses once its plan is known (reads: reads_per_seg): IOC_OK, or the status with the message set
static int ends_room_ok(ioc_ctx* c, const std::string& who, const EndsOut& o, const SinkPlan& p, const std::vector<int64_t>& reads)
{
    int64_t bound = 0, vbound = 0;
    for (size_t g = 0; g < p.segs.size(); ++g)
        bound += 2 * ends_sites_most(p.segs[g].rlen, o.rule.max_sites), vbound += ends_variants_most(reads[g], o.rule.max_variants);
    if (o.cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": sites_cap " + std::to_string(o.cap) + " below the bound " + std::to_string(bound));
    if (o.vcap < vbound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": variants_cap " + std::to_string(o.vcap) + " below the bound " + std::to_string(vbound));
    return (bound > 0 && !o.sites) || (vbound > 0 && !o.variants) || (!p.plane.empty() && !o.reads) || (!p.segs.empty() && !o.seg) ? IOC_ERR_ARG : IOC_OK;
}
static std::string ends_trace(const AlnTally& t)
{
    char buf[400];
    snprintf(buf, sizeof buf, "k_end_hist %.3f ms, k_end_rows %.3f ms, k_end_list %.3f ms, k_end_class %.3f ms, k_end_count %.3f ms, k_end_support %.3f ms, k_end_variants %.3f ms, k_ends_record %.3f ms",
             t.ms_ends[0], t.ms_ends[1], t.ms_ends[2], t.ms_ends[3], t.ms_ends[4], t.ms_ends[5], t.ms_ends[6], t.ms_ends[7]);
    return buf;
}

// upload -> ends -> copy-out.  The search for ends from extents the caller holds: they are uploaded, and the kernels run as behind
// ioc_align_pairs_blocks_ends.
int ioc_reads_ends(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, int32_t n_pairs, const int32_t* seg_of_pair, const ioc_read_extent* extents,
                   const int32_t* pre_group, int32_t slack, int32_t min_over, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites,
                   int32_t max_variants, ioc_end_row* out_rows, ioc_end_site* out_sites, int64_t sites_cap, int64_t* site_off, ioc_end_variant* out_variants,
                   int64_t variants_cap, int64_t* var_off, ioc_read_ends* out_reads, ioc_ends_seg* out_seg)
{
    const EndsOut o{{slack, min_over, min_depth, min_alt, min_pct, max_sites, max_variants}, out_rows, out_sites, sites_cap, site_off, out_variants, variants_cap,
                    var_off, out_reads, out_seg};
    if (!c || n_segs < 0 || n_pairs < 0 || !o.ok() || (n_segs > 0 && !rlen) || (n_pairs > 0 && (!seg_of_pair || !extents))) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen("ioc_reads_ends", n_segs, rlen, nullptr, nullptr, n_pairs, seg_of_pair, nullptr, PLAN_REFUSE_LONG)) return ioc_fail(c, st, p.msg);
    for (int32_t i = 0; i < n_pairs; ++i)
        if (!ends_extent_ok(extents[i], rlen[seg_of_pair[i]]) || (pre_group && pre_group[i] < -1))
            return ioc_fail(c, IOC_ERR_ARG, "ioc_reads_ends: the extent or pre_group of pair " + std::to_string(i) + " is outside its segment's range");
    IOC_TRY(ends_room_ok(c, "ioc_reads_ends", o, p, reads_per_seg(size_t(n_segs), size_t(n_pairs), seg_of_pair)));
    site_off[0] = 0, var_off[0] = 0;
    if (n_segs == 0) return IOC_OK;
    SinkRun r{c};
    IOC_TRY(r.ends(p, seg_of_pair, extents, pre_group, nullptr, 1, o));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   reads ends: %d segments, %lld rows, %d pairs, %lld sites kept, %lld variants kept, %s\n", n_segs, (long long)p.n_rows, n_pairs,
                (long long)site_off[2 * n_segs], (long long)var_off[n_segs], ends_trace(r.t).c_str());
    return IOC_OK;
}


// ---- the sequence of an inserted exon: the windows of the carriers at every kept site ----
namespace {
struct WindowsOut {  // the rule of a window call and where it leaves what it made (call.cap: what seq and qual hold each; call.off: sites + 1 entries)
    WinRule rule;
    CallOut call;
    ioc_insert_window* win;
    ioc_pileup_col* cols;
    ioc_pileup_ins* ins;
    bool ok() const { return rule.ok() && call.ok() && !cols == !ins; }
};
// the pairs' reads in the pool: where each begins and how long it is
struct WindowsReads {
    std::vector<int64_t> off;
    std::vector<uint32_t> len;
};
constexpr uint64_t WIN_DIR_WORDS_MOST = uint64_t(1) << 25;  // the direction words of one launch of k_win_align: 128 MB, 2048 alignments of 512 x 512

// what a window call refuses about its sites and its room: IOC_OK, or the status with the message set
static int windows_ok(ioc_ctx* c, const std::string& who, const WindowsOut& o, const SinkPlan& p, const ioc_pile_insert* sites, const int64_t* site_off, int64_t n_sites_most,
                      int64_t slots_a_site = 1)
{
    const size_t n = p.segs.size();
    if (site_off) {  // (the sites are the caller's: ioc_planes_insert_windows)
        if (site_off[0] != 0) return ioc_fail(c, IOC_ERR_ARG, who + ": site_off does not begin at 0");
        for (size_t g = 0; g < n; ++g) {
            if (site_off[g + 1] < site_off[g] || site_off[g + 1] - site_off[g] > IOC_INSERTS_MAX)
                return ioc_fail(c, IOC_ERR_ARG, who + ": segment " + std::to_string(g) + " has a negative number of sites or more than 32");
            for (int64_t x = site_off[g]; x < site_off[g + 1]; ++x)
                if (!sites || !win_site_ok(sites[x].first, sites[x].end, p.segs[g].rlen))
                    return ioc_fail(c, IOC_ERR_ARG, who + ": site " + std::to_string(x) + " does not lie inside its segment");
        }
        n_sites_most = site_off[n];
    }
    const int64_t bound = n_sites_most * slots_a_site * pile_call_most(o.rule.max_win);
    if (o.call.cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": cap " + std::to_string(o.call.cap) + " below the bound " + std::to_string(bound));
    return n_sites_most > 0 && (!o.win || !o.call.stats || !o.call.seq || !o.call.qual) ? IOC_ERR_ARG : IOC_OK;
}

// What k_win_bounds and k_win_template left of a call: a_windows' tables on the device — [segments][seg_of_pair][plane offsets][read
// lengths][member lists][sites][site_off][site_seg][keys], the (pair, site) entries and the records and, uploaded, the planes — and
// the records and the entries on the host.
struct WinTables {
    MemberLists m;
    std::vector<int32_t> site_seg;
    size_t stride = 1;
    IocWinDev v{};
    std::vector<ioc_insert_window> win;
    std::vector<IocWinSlot> slot;
    // what the entry of pair i at site k says, held against the read
    bool voter(const WindowsReads& reads, int32_t max_win, size_t i, size_t k, uint32_t& start, uint32_t& len) const
    {
        const IocWinSlot& s = slot[i * stride + k];
        start = s.start, len = win_slot_len(s.cls_len);
        return win_slot_class(s.cls_len) == uint32_t(IOC_WIN_VOTER) && len >= 1 && len <= uint32_t(max_win) && uint64_t(start) + len <= reads.len[i];
    }
};

// upload -> bounds -> template -> the records and the entries back.  The planes lie on the device (dev_*) or are the host's and
// uploaded; sites, site_off and keys are the host's.
static int windows_tables(SinkRun& r, const SinkPlan& pn, const int32_t* seg_of_pair, const WindowsReads& reads, const uint8_t* host_base, const uint32_t* host_qpos,
                          const uint8_t* dev_base, const uint32_t* dev_qpos, const ioc_pile_insert* sites, const int64_t* site_off, const uint64_t* keys,
                          const WinRule& rule, WinTables& t)
{
    ioc_ctx* const c = r.c;
    const size_t n = pn.segs.size(), np = pn.plane.size(), B = size_t(pn.plane_bytes), ns = size_t(site_off[n]);
    t.m = member_lists(n, np, seg_of_pair);
    t.site_seg = slot_owners(site_off, n);
    size_t stride = 1;
    for (size_t g = 0; g < n; ++g) stride = std::max(stride, size_t(site_off[g + 1] - site_off[g]));
    t.stride = stride;
    Arena l;
    const size_t o_seg = l.take(n * sizeof(IocPileSeg)), o_sop = l.take(np * 4), o_plane = l.take(np * 8), o_qlen = l.take(np * 4), o_moff = l.take((n + 1) * 4),
                 o_mem = l.take(np * 4), o_sites = l.take(ns * sizeof(ioc_pile_insert)), o_soff = l.take((n + 1) * 8), o_sseg = l.take(ns * 4),
                 o_keys = l.take(np * 8), tables = l.size();
    const size_t o_slots = l.take(np * stride * sizeof(IocWinSlot)), o_win = l.take(ns * sizeof(ioc_insert_window)), o_end = l.size(),
                 o_base = l.take(dev_base ? 0 : B), o_qpos = l.take(dev_qpos ? 0 : 4 * B);
    std::vector<uint8_t> stage(tables, 0);
    auto put = [&](size_t at, const void* src, size_t b) { if (b) memcpy(stage.data() + at, src, b); };
    put(o_seg, pn.segs.data(), n * sizeof(IocPileSeg)), put(o_sop, seg_of_pair, np * 4), put(o_plane, pn.plane.data(), np * 8), put(o_qlen, reads.len.data(), np * 4);
    put(o_moff, t.m.mem_off.data(), (n + 1) * 4), put(o_mem, t.m.members.data(), np * 4), put(o_sites, sites, ns * sizeof(ioc_pile_insert));
    put(o_soff, site_off, (n + 1) * 8), put(o_sseg, t.site_seg.data(), ns * 4), put(o_keys, keys, np * 8);
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_windows, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_windows.p);
    IOC_CHK(c, hipMemcpyAsync(p, stage.data(), tables, hipMemcpyHostToDevice, c->stream));
    if (!dev_base && B) IOC_CHK(c, hipMemcpyAsync(p + o_base, host_base, B, hipMemcpyHostToDevice, c->stream));
    if (!dev_qpos && B) IOC_CHK(c, hipMemcpyAsync(p + o_qpos, host_qpos, 4 * B, hipMemcpyHostToDevice, c->stream));
    if (o_end > o_slots) IOC_CHK(c, hipMemsetAsync(p + o_slots, 0, o_end - o_slots, c->stream));  // (the entries and the records)
    t.v = IocWinDev{reinterpret_cast<const IocPileSeg*>(p + o_seg), uint32_t(n), uint32_t(np), reinterpret_cast<const int32_t*>(p + o_sop),
                    reinterpret_cast<const uint64_t*>(p + o_plane), dev_base ? dev_base : p + o_base,
                    dev_qpos ? dev_qpos : reinterpret_cast<const uint32_t*>(p + o_qpos), uint64_t(B), reinterpret_cast<const uint32_t*>(p + o_qlen),
                    reinterpret_cast<const uint32_t*>(p + o_moff), reinterpret_cast<const uint32_t*>(p + o_mem), reinterpret_cast<const ioc_pile_insert*>(p + o_sites),
                    reinterpret_cast<const int64_t*>(p + o_soff), reinterpret_cast<const int32_t*>(p + o_sseg), uint32_t(ns),
                    reinterpret_cast<const unsigned long long*>(p + o_keys), reinterpret_cast<IocWinSlot*>(p + o_slots), uint32_t(stride), uint64_t(np * stride),
                    reinterpret_cast<ioc_insert_window*>(p + o_win)};
    KernelTimes each;
    IOC_TRY(each.create(c, 2));
    IOC_TRY(r.begin(r.t.ms_windows[0], !each.on()));
    IOC_CHK(c, iock_win_bounds_template(c->stream, t.v, rule.slack, rule.max_win, each.events()));
    IOC_TRY(r.end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    r.settled();
    each.add_to(r.t.ms_windows);
    t.win.assign(ns, ioc_insert_window{});
    t.slot.assign(np * stride, IocWinSlot{});
    return r.copy_out({{t.win.data(), p + o_win, ns * sizeof(ioc_insert_window)}, {t.slot.data(), p + o_slots, np * stride * sizeof(IocWinSlot)}});
}

// The alignments of one round of k_win_align, as the host lists them: an item each, its planes of tlen + 1 bytes one behind the
// other (P in all), its (pair, site) entry, and its direction words, of at most WIN_DIR_WORDS_MOST a launch.
struct WinRound {
    std::vector<IocWinItem> items;
    std::vector<uint64_t> vplane, entry;
    std::vector<size_t> launch{0};  // (the first item of every launch of k_win_align, and after close() the end)
    uint64_t P = 0, dir_at = 0, dir_most = 0;
    void add(uint64_t q_off, uint64_t t_off, uint32_t len, uint32_t t_len, uint64_t e)
    {
        const uint64_t words = win_dir_words(len, t_len);
        if (dir_at + words > WIN_DIR_WORDS_MOST) launch.push_back(items.size()), dir_at = 0;
        items.push_back(IocWinItem{q_off, t_off, P, dir_at, len, t_len});
        dir_at += words, dir_most = std::max(dir_most, dir_at);
        vplane.push_back(P), entry.push_back(e);
        P += uint64_t(t_len) + 1;
    }
    void close() { launch.push_back(items.size()); }
    bool fits() const { return items.size() <= size_t(INT32_MAX) && P <= (uint64_t(1) << 40); }
};
// where a round's blocks lie in its buffer: [items][base plane][slot planes][direction words]
struct WinRoundAt {
    size_t items, base, slots, dir;
    static WinRoundAt take(Arena& a, const WinRound& w)
    {
        WinRoundAt at;
        at.items = a.take(w.items.size() * sizeof(IocWinItem)), at.base = a.take(size_t(w.P)), at.slots = a.take(size_t(IOC_PILE_INS_SLOTS) * size_t(w.P)),
        at.dir = a.take(size_t(w.dir_most) * 4);
        return at;
    }
};
// the site's template, held against the entries: where its window lies in the pool and how long it is
static bool windows_template_at(const WinTables& t, const WindowsReads& reads, int32_t max_win, const int32_t* seg_of_pair, size_t g, size_t k, int32_t pair,
                                int32_t tlen, uint64_t& t_off, uint32_t& t_len)
{
    uint32_t t_start = 0;
    if (pair < 0 || size_t(pair) >= reads.len.size() || size_t(seg_of_pair[pair]) != g || !t.voter(reads, max_win, size_t(pair), k, t_start, t_len) || t_len != uint32_t(tlen))
        return false;
    t_off = uint64_t(reads.off[size_t(pair)]) + t_start;
    return true;
}
// upload the items -> set the planes -> k_win_align, launch after launch (`into`: what its device time is added to)
static int windows_align(SinkRun& r, uint8_t* q, const WinRoundAt& at, const WinRound& w, const WinRule& rule, double& into)
{
    ioc_ctx* const c = r.c;
    if (w.items.empty()) return IOC_OK;
    IOC_CHK(c, hipMemcpyAsync(q + at.items, w.items.data(), w.items.size() * sizeof(IocWinItem), hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemsetAsync(q + at.base, IOC_ALLELE_NONE, size_t(w.P), c->stream));
    IOC_CHK(c, hipMemsetAsync(q + at.slots, 0, size_t(IOC_PILE_INS_SLOTS) * size_t(w.P), c->stream));
    const uint8_t* pool = static_cast<const uint8_t*>(c->a_pool.p);
    const uint64_t pool_bytes = uint64_t(c->aln_offs.back());
    // (IOC_TRACE with IOC_WIN_SPLIT, for the measurement: the fill and the walk of every launch as two launches, timed apart; the
    // walk reads the words the fill left, so the planes are the same bytes)
    const bool split = getenv("IOC_TRACE") && getenv("IOC_WIN_SPLIT");
    for (size_t b = 0; b + 1 < w.launch.size(); ++b)
        for (int ph = split ? 1 : 0; ph <= (split ? 2 : 0); ++ph) {  // (0: both halves in one launch; 1, 2: the fill, then the walk)
            IOC_TRY(r.begin(ph == 2 ? r.t.ms_win_walk : into));
            IOC_CHK(c, iock_win_align(c->stream, reinterpret_cast<const IocWinItem*>(q + at.items) + w.launch[b], uint32_t(w.launch[b + 1] - w.launch[b]), pool, pool_bytes,
                                      q + at.base, q + at.slots, w.P, reinterpret_cast<uint32_t*>(q + at.dir), w.dir_most, rule.match, rule.mismatch, rule.gap, ph));
            IOC_TRY(r.end());
        }
    return IOC_OK;
}

// A site's template in a round and the round's items that are its voters', first .. end - 1 (t_len 0: the site has no round).
struct WinSite {
    uint64_t t_off = 0;
    uint32_t t_len = 0;
    size_t first = 0, end = 0;
};
// One round listed: for every site x that template_of(x, pair, tlen) gives a template, the members i of its segment that vote and
// that take(i, k) lets in, in pair order, against that template.  IOC_OK, or IOC_ERR_HIP where a template is no voter of its site.
// (no template: this stands inside extern "C" with the entry points)
static int windows_list_round(const WinTables& t, const WindowsReads& reads, int32_t max_win, const int32_t* seg_of_pair, const int64_t* site_off,
                              const std::function<bool(size_t, int32_t&, int32_t&)>& template_of, const std::function<bool(size_t, size_t)>& take,
                              std::vector<WinSite>& site, WinRound& round)
{
    site.assign(t.win.size(), WinSite{});
    for (size_t x = 0; x < t.win.size(); ++x) {
        const size_t g = size_t(t.site_seg[x]), k = x - size_t(site_off[g]);
        WinSite& s = site[x];
        s.first = s.end = round.items.size();
        int32_t pair = -1, tlen = 0;
        if (!template_of(x, pair, tlen)) continue;
        if (!windows_template_at(t, reads, max_win, seg_of_pair, g, k, pair, tlen, s.t_off, s.t_len)) return IOC_ERR_HIP;
        for (uint32_t mi = t.m.mem_off[g]; mi < t.m.mem_off[g + 1]; ++mi) {
            const size_t i = t.m.members[mi];
            uint32_t start = 0, len = 0;
            if (take(i, k) && t.voter(reads, max_win, i, k, start, len)) round.add(uint64_t(reads.off[i]) + start, s.t_off, len, s.t_len, uint64_t(i) * t.stride + k);
        }
        s.end = round.items.size();
    }
    round.close();
    return IOC_OK;
}
// What a packed call made of the group-segments y (off, st: a record each), spread over n_slots slots of which slot_of[y] is group-segment y's.
static void spread_called(const std::vector<int64_t>& off, const std::vector<ioc_polish_stats>& st, const size_t* slot_of, size_t n_slots, const CallOut& out)
{
    for (size_t y = 0, x = 0; x < n_slots; ++x) {
        const bool is = y < st.size() && slot_of[y] == x;
        out.off[x + 1] = out.off[x] + (is ? off[y + 1] - off[y] : 0);
        if (is) out.stats[x] = st[y++];
    }
}

// tables -> [the host lists the voters] -> align -> group pile -> call -> copy-out.  The host lists every called site's voters in pair
// order — an alignment each, a group of k_group_pile per site — and a_gpile holds the round's blocks (WinRoundAt) and [group-segments]
// [work items][plane offsets][gmem_off][gmembers][gcols][gins].
static int windows_device(SinkRun& r, const SinkPlan& pn, const int32_t* seg_of_pair, const WindowsReads& reads, const uint8_t* host_base, const uint32_t* host_qpos,
                   const uint8_t* dev_base, const uint32_t* dev_qpos, const ioc_pile_insert* sites, const int64_t* site_off, const uint64_t* keys,
                   const WindowsOut& o)
{
    ioc_ctx* const c = r.c;
    const size_t n = pn.segs.size(), ns = size_t(site_off[n]);
    for (size_t x = 0; x <= ns; ++x) o.call.off[x] = 0;
    for (size_t x = 0; x < ns; ++x) o.call.stats[x] = ioc_polish_stats{};
    if (ns == 0) return IOC_OK;
    WinTables t;
    IOC_TRY(windows_tables(r, pn, seg_of_pair, reads, host_base, host_qpos, dev_base, dev_qpos, sites, site_off, keys, o.rule, t));

    // every called site's voters, in pair order: an alignment each; the site is a group-segment of tlen + 1 rows
    std::vector<IocPileSeg> gsegs;
    std::vector<uint32_t> goff{0}, gmem;
    WinRound round;
    std::vector<WinSite> site;
    std::vector<IocGroupWork> work;
    std::vector<size_t> called;
    int64_t rows = 0;
    if (windows_list_round(t, reads, o.rule.max_win, seg_of_pair, site_off,
                           [&](size_t x, int32_t& pair, int32_t& tlen) { return pair = t.win[x].template_pair, (tlen = t.win[x].tlen) > 0; },
                           [](size_t, size_t) { return true; }, site, round))
        return ioc_fail(c, IOC_ERR_HIP, "the window kernels returned a template that is no voter of its site");
    for (size_t x = 0; x < ns; ++x) {
        const WinSite& w = site[x];
        if (w.t_len == 0) continue;
        for (size_t y = w.first; y < w.end; ++y) gmem.push_back(uint32_t(y));
        for (int64_t row = 0; row <= int64_t(w.t_len); row += IOC_GROUP_PILE_ROWS) work.push_back(IocGroupWork{uint32_t(gsegs.size()), uint32_t(row)});
        gsegs.push_back(IocPileSeg{rows, int64_t(w.t_off), int32_t(w.t_len), 0});
        goff.push_back(uint32_t(gmem.size()));
        rows += int64_t(w.t_len) + 1;
        called.push_back(x);
    }
    std::copy(t.win.begin(), t.win.end(), o.win);
    if (called.empty()) return IOC_OK;
    if (!round.fits()) return ioc_fail(c, IOC_ERR_CAPACITY, "the windows of the call have more than 2^31 - 1 voters");

    const size_t G = gsegs.size(), M = round.items.size();
    Arena a;
    const WinRoundAt at = WinRoundAt::take(a, round);
    const size_t a_gseg = a.take(G * sizeof(IocPileSeg)), a_work = a.take(work.size() * sizeof(IocGroupWork)), a_plane = a.take(M * 8), a_goff = a.take((G + 1) * 4),
                 a_gmem = a.take(M * 4), a_cols = a.take(size_t(rows) * sizeof(ioc_pileup_col)), a_ins = a.take(size_t(rows) * sizeof(ioc_pileup_ins)), a_end = a.size();
    IOC_TRY(ioc_reserve(c, c->a_gpile, a.size()));
    uint8_t* q = static_cast<uint8_t*>(c->a_gpile.p);
    auto up = [&](size_t at_, const void* src, size_t b) { return b ? hipMemcpyAsync(q + at_, src, b, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
    IOC_CHK(c, up(a_gseg, gsegs.data(), G * sizeof(IocPileSeg)));
    IOC_CHK(c, up(a_work, work.data(), work.size() * sizeof(IocGroupWork)));
    IOC_CHK(c, up(a_plane, round.vplane.data(), M * 8));
    IOC_CHK(c, up(a_goff, goff.data(), (G + 1) * 4));
    IOC_CHK(c, up(a_gmem, gmem.data(), M * 4));
    IOC_CHK(c, hipMemsetAsync(q + a_cols, 0, a_end - a_cols, c->stream));  // (both tables)
    IOC_TRY(windows_align(r, q, at, round, o.rule, r.t.ms_windows[2]));
    const uint8_t* pool = static_cast<const uint8_t*>(c->a_pool.p);
    const uint64_t pool_bytes = uint64_t(c->aln_offs.back());
    ioc_pileup_col* const d_cols = reinterpret_cast<ioc_pileup_col*>(q + a_cols);
    ioc_pileup_ins* const d_ins = reinterpret_cast<ioc_pileup_ins*>(q + a_ins);
    IOC_TRY(r.begin(r.t.ms_windows[3]));
    IOC_CHK(c, iock_group_pile(c->stream, reinterpret_cast<const IocGroupWork*>(q + a_work), uint32_t(work.size()), reinterpret_cast<const IocPileSeg*>(q + a_gseg),
                               uint32_t(G), reinterpret_cast<const uint32_t*>(q + a_goff), reinterpret_cast<const uint32_t*>(q + a_gmem), uint32_t(M), uint32_t(M),
                               reinterpret_cast<const uint64_t*>(q + a_plane), q + at.base, q + at.slots, round.P, d_cols, d_ins, uint64_t(rows)));
    IOC_TRY(r.end());
    std::vector<int64_t> off(G + 1, 0);
    std::vector<ioc_polish_stats> st(G);
    const CallOut packed{o.call.min_depth, o.call.seq, o.call.qual, o.call.cap, off.data(), st.data()};  // (the called sites' bytes are all sites' bytes, packed)
    IOC_TRY(pile_call_device(r, gsegs, pool, pool_bytes, packed, d_cols, d_ins, nullptr, rows));
    spread_called(off, st, called.data(), ns, o.call);
    return r.copy_out({{o.cols, d_cols, size_t(rows) * sizeof(ioc_pileup_col)}, {o.ins, d_ins, size_t(rows) * sizeof(ioc_pileup_ins)}});
}

static std::string windows_trace(const AlnTally& t)
{
    char buf[240];
    snprintf(buf, sizeof buf, "k_win_bounds %.3f ms, k_win_template %.3f ms, k_win_align %.3f ms, k_win_align_walk %.3f ms, k_win_group_pile %.3f ms, k_win_pile_call %.3f ms",
             t.ms_windows[0], t.ms_windows[1], t.ms_windows[2], t.ms_win_walk, t.ms_windows[3], t.ms_call);
    return buf;
}
// ---- two exons at one junction: the variants of the kept sites ----
struct VariantsOut {  // the rule of a variant call beside the window rule, and where it leaves what it made beside the windows' outputs
    WinVarRule rule;
    ioc_window_variant* var;
    uint8_t* variant;   // IOC_INSERTS_MAX bytes a pair
    int32_t* agree;     // (may be NULL) 2 IOC_INSERTS_MAX words a pair
    ioc_read_variants* reads;
    ioc_variants_seg* seg;
};

struct VariantsFused {  // the variant stage behind the insert stage (ioc_align_pairs_blocks_inserts_variants): its rule and outputs, and its slots' bytes
    VariantsOut vo;
    CallOut call;
};

// One round of the variant stage where it lies on the device: the host's list, its sites, the buffer its blocks are in and where.
struct VariantRound {
    WinRound w;
    std::vector<WinSite> site;
    uint8_t* q = nullptr;
    WinRoundAt at{};
};

// The slots of a variant call: a group-segment per (called site, variant that has one), its members the items of its round whose voter
// is of the variant — round B's items count from round A's last —, the work items of either round's launch of k_group_pile, and
// slot_of, the slot 2 x + h of every group-segment.  With `with_all` (the fused call) the window call's own sites stand behind the
// n_slots slots: every item of round A, all voters voting.
struct VariantSlots {
    std::vector<IocPileSeg> gsegs;
    std::vector<uint32_t> goff{0}, gmem;
    std::vector<IocGroupWork> work_a, work_b;
    std::vector<size_t> slot_of;
    int64_t rows = 0;
    size_t n_slots = 0;
    void add(size_t slot, const WinSite& st, const WinRound& w, size_t item0, const std::vector<uint8_t>* variant, uint8_t which, std::vector<IocGroupWork>& work)
    {
        for (size_t y = st.first; y < st.end; ++y)
            if (!variant || (*variant)[size_t(w.entry[y])] == which) gmem.push_back(uint32_t(item0 + y));
        for (int64_t row = 0; row <= int64_t(st.t_len); row += IOC_GROUP_PILE_ROWS) work.push_back(IocGroupWork{uint32_t(gsegs.size()), uint32_t(row)});
        gsegs.push_back(IocPileSeg{rows, int64_t(st.t_off), int32_t(st.t_len), 0});
        goff.push_back(uint32_t(gmem.size()));
        rows += int64_t(st.t_len) + 1;
        slot_of.push_back(slot);
    }
    static VariantSlots list(const VariantRound& ra, const VariantRound& rb, const std::vector<ioc_window_variant>& var, const std::vector<uint8_t>& variant, bool with_all)
    {
        VariantSlots v;
        const size_t ns = var.size(), MA = ra.w.items.size();
        for (size_t x = 0; x < ns; ++x) {
            if (ra.site[x].t_len > 0) v.add(2 * x, ra.site[x], ra.w, 0, &variant, uint8_t(IOC_WINVAR_A), v.work_a);
            if (var[x].split && rb.site[x].t_len > 0) v.add(2 * x + 1, rb.site[x], rb.w, MA, &variant, uint8_t(IOC_WINVAR_B), v.work_b);
        }
        v.n_slots = v.gsegs.size();
        for (size_t x = 0; x < ns && with_all; ++x)
            if (ra.site[x].t_len > 0) v.add(x, ra.site[x], ra.w, 0, nullptr, 0, v.work_a);
        return v;
    }
};
// what the slots may need at most, known once round B is listed: every site of round B splitting
struct VariantSlotsMost {
    size_t slots = 0, work = 0, members = 0;
    int64_t rows = 0;
    void add(const WinSite& s) { ++slots, rows += int64_t(s.t_len) + 1, work += s.t_len / IOC_GROUP_PILE_ROWS + 1; }
    bool holds(const VariantSlots& v) const { return v.gsegs.size() <= slots && v.rows <= rows && v.work_a.size() + v.work_b.size() <= work && v.gmem.size() <= members; }
};
// where the slots' blocks lie in round B's buffer, behind its own: [group-segments][work items][plane offsets][gmem_off][gmembers][gcols][gins]
struct VariantSlotsAt {
    size_t gseg, work, plane, goff, gmem, cols, ins, end;
    static VariantSlotsAt take(Arena& b, const VariantSlotsMost& most, size_t items)
    {
        VariantSlotsAt at;
        at.gseg = b.take(most.slots * sizeof(IocPileSeg)), at.work = b.take(most.work * sizeof(IocGroupWork)), at.plane = b.take(items * 8);
        at.goff = b.take((most.slots + 1) * 4), at.gmem = b.take(most.members * 4), at.cols = b.take(size_t(most.rows) * sizeof(ioc_pileup_col));
        at.ins = b.take(size_t(most.rows) * sizeof(ioc_pileup_ins)), at.end = b.size();
        return at;
    }
};

// upload the slots -> group pile, a launch a round (a member's plane offset counts from its own round's planes) -> call the slots ->
// call the window call's own sites behind them (all; NULL: there are none).
static int variants_call_slots(SinkRun& r, const VariantSlots& v, const VariantSlotsAt& at, const VariantRound& ra, const VariantRound& rb, const CallOut& slots,
                               size_t n_sites, const CallOut* all)
{
    ioc_ctx* const c = r.c;
    const size_t G = v.n_slots, MA = ra.w.items.size(), MB = rb.w.items.size();
    if (G == 0) return IOC_OK;
    uint8_t* const qb = rb.q;
    std::vector<uint64_t> vplane(ra.w.vplane);
    vplane.insert(vplane.end(), rb.w.vplane.begin(), rb.w.vplane.end());
    auto up = [&](size_t at_, const void* src, size_t b) { return b ? hipMemcpyAsync(qb + at_, src, b, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
    IOC_CHK(c, up(at.gseg, v.gsegs.data(), v.gsegs.size() * sizeof(IocPileSeg)));
    IOC_CHK(c, up(at.work, v.work_a.data(), v.work_a.size() * sizeof(IocGroupWork)));
    IOC_CHK(c, up(at.work + v.work_a.size() * sizeof(IocGroupWork), v.work_b.data(), v.work_b.size() * sizeof(IocGroupWork)));
    IOC_CHK(c, up(at.plane, vplane.data(), (MA + MB) * 8));
    IOC_CHK(c, up(at.goff, v.goff.data(), v.goff.size() * 4));
    IOC_CHK(c, up(at.gmem, v.gmem.data(), v.gmem.size() * 4));
    IOC_CHK(c, hipMemsetAsync(qb + at.cols, 0, at.end - at.cols, c->stream));  // (both tables)
    ioc_pileup_col* const d_cols = reinterpret_cast<ioc_pileup_col*>(qb + at.cols);
    ioc_pileup_ins* const d_ins = reinterpret_cast<ioc_pileup_ins*>(qb + at.ins);
    const IocGroupWork* const d_work = reinterpret_cast<const IocGroupWork*>(qb + at.work);
    auto pile = [&](const IocGroupWork* work, size_t n_work, const VariantRound& of) {
        return iock_group_pile(c->stream, work, uint32_t(n_work), reinterpret_cast<const IocPileSeg*>(qb + at.gseg), uint32_t(v.gsegs.size()),
                               reinterpret_cast<const uint32_t*>(qb + at.goff), reinterpret_cast<const uint32_t*>(qb + at.gmem), uint32_t(v.gmem.size()), uint32_t(MA + MB),
                               reinterpret_cast<const uint64_t*>(qb + at.plane), of.q + of.at.base, of.q + of.at.slots, of.w.P, d_cols, d_ins, uint64_t(v.rows));
    };
    IOC_TRY(r.begin(r.t.ms_windows[3]));
    IOC_CHK(c, pile(d_work, v.work_a.size(), ra));
    if (!v.work_b.empty()) IOC_CHK(c, pile(d_work + v.work_a.size(), v.work_b.size(), rb));
    IOC_TRY(r.end());
    const uint8_t* pool = static_cast<const uint8_t*>(c->a_pool.p);
    const uint64_t pool_bytes = uint64_t(c->aln_offs.back());
    // (the called slots' bytes are all slots' bytes, packed; and so are the sites')
    auto call = [&](size_t first, size_t end, size_t n_out, const CallOut& out) {
        std::vector<int64_t> off(end - first + 1, 0);
        std::vector<ioc_polish_stats> st(end - first);
        const CallOut packed{out.min_depth, out.seq, out.qual, out.cap, off.data(), st.data()};
        IOC_TRY(pile_call_device(r, std::vector<IocPileSeg>(v.gsegs.begin() + int64_t(first), v.gsegs.begin() + int64_t(end)), pool, pool_bytes, packed, d_cols, d_ins, nullptr,
                                 v.rows));
        spread_called(off, st, v.slot_of.data() + first, n_out, out);
        return int(IOC_OK);
    };
    IOC_TRY(call(0, G, 2 * n_sites, slots));
    if (all && v.gsegs.size() > G) IOC_TRY(call(G, v.gsegs.size(), n_sites, *all));
    return IOC_OK;
}

// tables -> [round A listed] -> align -> agree -> template B -> [round B listed] -> align -> agree -> decide -> rekey -> the isoforms
// again -> [the slots listed] -> group pile -> call -> copy-out.  o.call: 2 sites slots (off: 2 sites + 1 entries), slot 2 x site x's
// variant A and 2 x + 1 its B.  Round A lies in a_gpile as the window call has it; a_winvar holds [round A's entries][pre_key]
// [pre_mask][pre_full], the flags, agreements, records and variant bytes and the recount's records; a_winvar_b round B's blocks and
// entries and the slots' (VariantSlotsAt).  all (the fused call; else NULL): where the window call's own consensus of every site goes,
// all voters voting — one more group-segment a called site over round A's planes, piled with the slots and called behind them.
static int variants_device(SinkRun& r, const SinkPlan& pn, const int32_t* seg_of_pair, const WindowsReads& reads, const uint8_t* host_base, const uint32_t* host_qpos,
                           const uint8_t* dev_base, const uint32_t* dev_qpos, const ioc_pile_insert* sites, const int64_t* site_off, const uint64_t* keys,
                           const uint64_t* pre_key, const uint64_t* pre_mask, const uint64_t* pre_full, const WindowsOut& o, const VariantsOut& vo,
                           const CallOut* all = nullptr)
{
    ioc_ctx* const c = r.c;
    const size_t n = pn.segs.size(), np = pn.plane.size(), ns = size_t(site_off[n]), S = size_t(IOC_INSERTS_MAX);
    for (size_t x = 0; x <= 2 * ns; ++x) o.call.off[x] = 0;
    for (size_t x = 0; x < 2 * ns; ++x) o.call.stats[x] = ioc_polish_stats{};
    for (size_t x = 0; x <= ns && all; ++x) all->off[x] = 0;
    for (size_t x = 0; x < ns && all; ++x) all->stats[x] = ioc_polish_stats{};
    if (n == 0) return IOC_OK;
    WinTables t;
    IOC_TRY(windows_tables(r, pn, seg_of_pair, reads, host_base, host_qpos, dev_base, dev_qpos, sites, site_off, keys, o.rule, t));
    const size_t E = np * t.stride;  // the (pair, site) entries

    // round A: every called site's voters against its template
    VariantRound ra, rb;
    if (windows_list_round(t, reads, o.rule.max_win, seg_of_pair, site_off,
                           [&](size_t x, int32_t& pair, int32_t& tlen) { return pair = t.win[x].template_pair, (tlen = t.win[x].tlen) > 0; },
                           [](size_t, size_t) { return true; }, ra.site, ra.w))
        return ioc_fail(c, IOC_ERR_HIP, "the window kernels returned a template that is no voter of its site");
    if (!ra.w.fits()) return ioc_fail(c, IOC_ERR_CAPACITY, "the windows of the call have more than 2^31 - 1 voters");
    Arena a;
    ra.at = WinRoundAt::take(a, ra.w);
    IOC_TRY(ioc_reserve(c, c->a_gpile, a.size()));
    ra.q = static_cast<uint8_t*>(c->a_gpile.p);
    IOC_TRY(windows_align(r, ra.q, ra.at, ra.w, o.rule, r.t.ms_windows[2]));

    const size_t MA = ra.w.items.size();
    const bool with_pre = pre_key != nullptr;  // (all three or none: the entry point has seen to it)
    Arena l;
    const size_t o_at = l.take(MA * 8), o_pk = l.take(with_pre ? np * 8 : 0), o_pm = l.take(with_pre ? np * 8 : 0), o_pf = l.take(with_pre ? n * 8 : 0);
    const size_t o_flag = l.take(2 * E), o_var = l.take(ns * sizeof(ioc_window_variant)), o_variant = l.take(E), o_reads = l.take(np * sizeof(ioc_read_inserts)),
                 o_mask = l.take(np * 8), o_kflags = l.take(np), o_rec = l.take(n * sizeof(ioc_variants_seg)), o_zend = l.size(), o_agree = l.take(2 * E * 4);
    IOC_TRY(ioc_reserve(c, c->a_winvar, l.size()));
    uint8_t* const p = static_cast<uint8_t*>(c->a_winvar.p);
    auto up = [&](uint8_t* base, size_t at_, const void* src, size_t b) { return b ? hipMemcpyAsync(base + at_, src, b, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
    IOC_CHK(c, up(p, o_at, ra.w.entry.data(), MA * 8));
    if (with_pre) {
        IOC_CHK(c, up(p, o_pk, pre_key, np * 8));
        IOC_CHK(c, up(p, o_pm, pre_mask, np * 8));
        IOC_CHK(c, up(p, o_pf, pre_full, n * 8));
    }
    if (o_zend > o_flag) IOC_CHK(c, hipMemsetAsync(p + o_flag, 0, o_zend - o_flag, c->stream));  // (the flags, the records, the variant bytes and the recount's)
    if (E) IOC_CHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p + o_agree), int(INT32_MIN), 2 * E, c->stream));
    const IocWinVarDev v{t.v, p + o_flag, reinterpret_cast<int32_t*>(p + o_agree), reinterpret_cast<ioc_window_variant*>(p + o_var), p + o_variant};
    const uint8_t* pool = static_cast<const uint8_t*>(c->a_pool.p);
    const uint64_t pool_bytes = uint64_t(c->aln_offs.back());
    auto agree_round = [&](const VariantRound& of, const uint64_t* d_at, size_t which) {
        return iock_win_agree(c->stream, reinterpret_cast<const IocWinItem*>(of.q + of.at.items), d_at, uint32_t(of.w.items.size()), pool, pool_bytes, of.q + of.at.base,
                              of.w.P, v.agree + which * E, v.flag + which * E, uint64_t(E), vo.rule.min_agree);
    };
    IOC_TRY(r.begin(r.t.ms_winvar[0]));
    IOC_CHK(c, agree_round(ra, reinterpret_cast<const uint64_t*>(p + o_at), 0));
    IOC_TRY(r.end());
    IOC_TRY(r.begin(r.t.ms_winvar[1]));
    IOC_CHK(c, iock_win_template_far(c->stream, v, vo.rule));
    IOC_TRY(r.end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    r.settled();
    std::vector<ioc_window_variant> var(ns);
    std::vector<uint8_t> flag_a(E);
    IOC_TRY(r.copy_out({{var.data(), p + o_var, ns * sizeof(ioc_window_variant)}, {flag_a.data(), p + o_flag, E}}));

    // round B: the far voters of the sites that reach it against template B; and what the slots may need at most
    auto far = [&](size_t i, size_t k) { return flag_a[i * t.stride + k] == WINVAR_FAR; };
    if (windows_list_round(t, reads, o.rule.max_win, seg_of_pair, site_off,
                           [&](size_t x, int32_t& pair, int32_t& tlen) { return pair = var[x].template_pair_b, tlen = var[x].tlen_b, pair >= 0; }, far, rb.site, rb.w))
        return ioc_fail(c, IOC_ERR_HIP, "the variant kernels returned a template B that is no voter of its site");
    VariantSlotsMost most;
    for (size_t x = 0; x < ns; ++x) {
        const size_t g = size_t(t.site_seg[x]), k = x - size_t(site_off[g]);
        if (rb.site[x].t_len > 0 && (ra.site[x].t_len == 0 || !far(size_t(var[x].template_pair_b), k)))
            return ioc_fail(c, IOC_ERR_HIP, "the variant kernels returned a template B that is no far voter of its site");
        if (ra.site[x].t_len > 0) most.add(ra.site[x]);
        if (ra.site[x].t_len > 0 && all) most.add(ra.site[x]);
        if (rb.site[x].t_len > 0) most.add(rb.site[x]);
    }
    const size_t MB = rb.w.items.size();
    most.members = 2 * MA + MB;
    r.t.win_voters += int64_t(MA), r.t.win_voters_b += int64_t(MB);
    Arena b;
    rb.at = WinRoundAt::take(b, rb.w);
    const size_t b_at = b.take(MB * 8);
    const VariantSlotsAt slots_at = VariantSlotsAt::take(b, most, MA + MB);
    IOC_TRY(ioc_reserve(c, c->a_winvar_b, b.size()));
    rb.q = static_cast<uint8_t*>(c->a_winvar_b.p);
    IOC_CHK(c, up(rb.q, b_at, rb.w.entry.data(), MB * 8));
    IOC_TRY(windows_align(r, rb.q, rb.at, rb.w, o.rule, r.t.ms_winvar[2]));
    IOC_TRY(r.begin(r.t.ms_winvar[0]));
    IOC_CHK(c, agree_round(rb, reinterpret_cast<const uint64_t*>(rb.q + b_at), 1));
    IOC_TRY(r.end());

    // decide -> rekey -> the isoforms again
    IocReadInsertsDev kv{};
    kv.n_segs = uint32_t(n), kv.n_pairs = uint32_t(np), kv.seg_of_pair = t.v.seg_of_pair, kv.mem_off = t.v.mem_off, kv.members = t.v.members;
    if (with_pre) {
        kv.pre_key = reinterpret_cast<const unsigned long long*>(p + o_pk), kv.pre_mask = reinterpret_cast<const unsigned long long*>(p + o_pm);
        kv.pre_full = reinterpret_cast<const unsigned long long*>(p + o_pf);
    }
    kv.pre_key_stride = kv.pre_mask_stride = 1;
    kv.mask = reinterpret_cast<unsigned long long*>(p + o_mask), kv.flags = p + o_kflags, kv.reads = reinterpret_cast<ioc_read_inserts*>(p + o_reads);
    KernelTimes each;
    IOC_TRY(each.create(c, IOC_WIN_VARIANTS_KERNELS));
    IOC_TRY(r.begin(r.t.ms_winvar[3], !each.on()));
    IOC_CHK(c, iock_win_decide_rekey(c->stream, v, vo.rule, kv, reinterpret_cast<ioc_variants_seg*>(p + o_rec), each.events()));
    IOC_TRY(r.end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    r.settled();
    each.add_to(r.t.ms_winvar + 3);
    std::vector<uint8_t> variant(E);
    std::vector<int32_t> agree(vo.agree ? 2 * E : 0);
    std::vector<ioc_read_inserts> rec(np);
    IOC_TRY(r.copy_out({{var.data(), p + o_var, ns * sizeof(ioc_window_variant)}, {variant.data(), p + o_variant, E}, {rec.data(), p + o_reads, np * sizeof(ioc_read_inserts)},
                        {vo.seg, p + o_rec, n * sizeof(ioc_variants_seg)}, {vo.agree ? agree.data() : nullptr, p + o_agree, 2 * E * 4}}));
    for (size_t i = 0; i < np; ++i) {  // (the entries are `stride` a pair on the device, IOC_INSERTS_MAX a pair for the caller)
        const size_t g = size_t(seg_of_pair[i]), kept = size_t(site_off[g + 1] - site_off[g]);
        vo.reads[i] = ioc_read_variants{rec[i].key, rec[i].group, rec[i].how};
        for (size_t k = 0; k < S; ++k) {
            vo.variant[i * S + k] = k < kept ? variant[i * t.stride + k] : uint8_t(IOC_WINVAR_NONE);
            for (size_t h = 0; h < 2 && vo.agree; ++h) vo.agree[(i * S + k) * 2 + h] = k < kept ? agree[h * E + i * t.stride + k] : INT32_MIN;
        }
    }
    std::copy(t.win.begin(), t.win.end(), o.win);
    std::copy(var.begin(), var.end(), vo.var);

    const VariantSlots slots = VariantSlots::list(ra, rb, var, variant, all != nullptr);
    if (!most.holds(slots)) return ioc_fail(c, IOC_ERR_HIP, "the variant kernels returned more slots than the sites of round B allow");
    return variants_call_slots(r, slots, slots_at, ra, rb, o.call, ns, all);
}

static std::string variants_trace(const AlnTally& t)
{
    char buf[400];
    snprintf(buf, sizeof buf, "k_win_agree %.3f ms, k_win_template_far %.3f ms, k_win_align_b %.3f ms, k_win_decide %.3f ms, k_win_rekey %.3f ms, k_winvar_support %.3f ms, "
             "k_winvar_isoforms %.3f ms, k_winvar_record %.3f ms, %lld voters, %lld of them in round B",
             t.ms_winvar[0], t.ms_winvar[1], t.ms_winvar[2], t.ms_winvar[3], t.ms_winvar[4], t.ms_winvar[5], t.ms_winvar[6], t.ms_winvar[7], (long long)t.win_voters,
             (long long)t.win_voters_b);
    return buf;
}
}  // namespace

// upload -> windows -> copy-out.  The windows from planes, sites and keys the caller holds, over the pool that is set.
int ioc_planes_insert_windows(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* query, const uint8_t* base,
                              const uint32_t* qpos, const ioc_pile_insert* sites, const int64_t* site_off, const uint64_t* keys, int32_t slack, int32_t max_win,
                              int32_t match, int32_t mismatch, int32_t gap, int32_t polish_min_depth, ioc_insert_window* out_win, char* out_seq, char* out_qual,
                              int64_t cap, int64_t* out_off, ioc_polish_stats* out_stats, ioc_pileup_col* out_cols, ioc_pileup_ins* out_ins)
{
    const std::string who = "ioc_planes_insert_windows";
    const WindowsOut o{{slack, max_win, match, mismatch, gap}, {polish_min_depth, out_seq, out_qual, cap, out_off, out_stats}, out_win, out_cols, out_ins};
    if (!c || n_segs < 0 || n_pairs < 0 || !o.ok() || !site_off || (n_segs > 0 && !rlen) || (n_pairs > 0 && (!seg_of_pair || !query || !keys))) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen(who, n_segs, rlen, nullptr, nullptr, n_pairs, seg_of_pair, nullptr, 0)) return ioc_fail(c, st, p.msg);
    if (p.plane_bytes > 0 && (!base || !qpos)) return IOC_ERR_ARG;
    WindowsReads reads;
    for (int32_t i = 0; i < n_pairs; ++i) {
        if (query[i] < 0 || size_t(query[i]) + 1 >= c->aln_offs.size()) return ioc_fail(c, IOC_ERR_ARG, who + ": the read of pair " + std::to_string(i) + " lies outside the pool");
        reads.off.push_back(c->aln_offs[size_t(query[i])]), reads.len.push_back(uint32_t(ioc_seq_len(c, query[i])));
    }
    IOC_TRY(windows_ok(c, who, o, p, sites, site_off, 0));
    SinkRun r{c};
    IOC_TRY(windows_device(r, p, seg_of_pair, reads, base, qpos, nullptr, nullptr, sites, site_off, keys, o));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes insert windows: %d segments, %d pairs, %lld sites, %lld bytes called, %s\n", n_segs, n_pairs, (long long)site_off[n_segs],
                (long long)out_off[site_off[n_segs]], windows_trace(r.t).c_str());
    return IOC_OK;
}

// upload -> windows and variants -> copy-out.  From planes, sites and keys the caller holds, over the pool that is set.
int ioc_planes_insert_window_variants(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* query,
                                      const uint8_t* base, const uint32_t* qpos, const ioc_pile_insert* sites, const int64_t* site_off, const uint64_t* keys, int32_t slack,
                                      int32_t max_win, int32_t match, int32_t mismatch, int32_t gap, int32_t polish_min_depth, int32_t min_agree, int32_t min_alt,
                                      int32_t min_pct, const uint64_t* pre_key, const uint64_t* pre_mask, const uint64_t* pre_full, ioc_insert_window* out_win,
                                      ioc_window_variant* out_var, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_stats,
                                      uint8_t* out_variant, int32_t* out_agree, ioc_read_variants* out_reads, ioc_variants_seg* out_seg)
{
    const std::string who = "ioc_planes_insert_window_variants";
    const WindowsOut o{{slack, max_win, match, mismatch, gap}, {polish_min_depth, out_seq, out_qual, cap, out_off, out_stats}, out_win, nullptr, nullptr};
    const VariantsOut vo{{min_agree, min_alt, min_pct}, out_var, out_variant, out_agree, out_reads, out_seg};
    const bool some_pre = pre_key || pre_mask || pre_full, all_pre = pre_key && pre_mask && pre_full;
    if (!c || n_segs < 0 || n_pairs < 0 || !o.ok() || !vo.rule.ok() || !site_off || (n_segs > 0 && (!rlen || !out_seg)) ||
        (n_pairs > 0 && (!seg_of_pair || !query || !keys || !out_variant || !out_reads)) || (some_pre && !all_pre))
        return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen(who, n_segs, rlen, nullptr, nullptr, n_pairs, seg_of_pair, nullptr, 0)) return ioc_fail(c, st, p.msg);
    if (p.plane_bytes > 0 && (!base || !qpos)) return IOC_ERR_ARG;
    WindowsReads reads;
    for (int32_t i = 0; i < n_pairs; ++i) {
        if (query[i] < 0 || size_t(query[i]) + 1 >= c->aln_offs.size()) return ioc_fail(c, IOC_ERR_ARG, who + ": the read of pair " + std::to_string(i) + " lies outside the pool");
        reads.off.push_back(c->aln_offs[size_t(query[i])]), reads.len.push_back(uint32_t(ioc_seq_len(c, query[i])));
    }
    IOC_TRY(windows_ok(c, who, o, p, sites, site_off, 0, /*slots a site*/ 2));
    if (site_off[n_segs] > 0 && !out_var) return IOC_ERR_ARG;
    SinkRun r{c};
    IOC_TRY(variants_device(r, p, seg_of_pair, reads, base, qpos, nullptr, nullptr, sites, site_off, keys, pre_key, pre_mask, pre_full, o, vo));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes insert window variants: %d segments, %d pairs, %lld sites, %lld bytes called, %s, %s\n", n_segs, n_pairs, (long long)site_off[n_segs],
                (long long)out_off[2 * site_off[n_segs]], windows_trace(r.t).c_str(), variants_trace(r.t).c_str());
    return IOC_OK;
}

namespace {
// what a splice reads beside the group tables, all the host's: a key per group-segment, the segments' window records packed with
// site_off, their called bytes packed with win_off.  by_variant (ioc_host_isoform_splice_variants): the keys are key2, `var` holds a
// record per site beside `win`, and wseq / wqual / win_off are the variant stage's slots, two a site (2 site_off[n] + 1 offsets).
struct SpliceIn {
    const uint64_t* keys;
    const ioc_insert_window* win;
    const int64_t* site_off;
    const char *wseq, *wqual;
    const int64_t* win_off;
    const ioc_window_variant* var = nullptr;
    bool by_variant = false;
    // the fused call's room counts one slot a site, the longer one: an isoform takes one, and the caller's cap was checked against one
    // window's most a site before anything ran — so no refusal comes after the stages have written.  The planes entry keeps the
    // definition's rule, the bytes of all slots.
    bool longer_slot_room = false;
    int64_t per_site() const { return by_variant ? 2 : 1; }
    int64_t room(int64_t s0, int64_t s1) const  // what the windows of sites s0 .. s1 add to an isoform's bound
    {
        if (!longer_slot_room) return win_off[per_site() * s1] - win_off[per_site() * s0];
        int64_t sum = 0;
        for (int64_t x = s0; x < s1; ++x) sum += std::max(win_off[2 * x + 1] - win_off[2 * x], win_off[2 * x + 2] - win_off[2 * x + 1]);
        return sum;
    }
};
struct SpliceOut {  // where a splice leaves what it made (call.off: G + 1 entries; cap: the records `splice` holds; splice_off: G + 1 entries)
    CallOut call;
    ioc_splice_stats* sstats;
    ioc_splice_site* splice;
    int64_t cap;
    int64_t* splice_off;
    bool ok() const { return call.ok() && splice_off && cap >= 0; }
};

// what a splice over n_groups[g] group-segments of segment g refuses about its windows and its room: IOC_OK, or the status with the
// message set.  The bound is the sum over the segments of n_groups[g] * (pile_call_most(rlen[g]) + the bytes of g's windows).
static int splice_ok(ioc_ctx* c, const std::string& who, const SpliceIn& in, const SpliceOut& o, const std::vector<IocPileSeg>& ds, const int32_t* n_groups, int64_t* out_bound)
{
    const size_t n = ds.size();
    if (!in.site_off || !in.win_off) return IOC_ERR_ARG;
    if (in.site_off[0] != 0 || in.win_off[0] != 0) return ioc_fail(c, IOC_ERR_ARG, who + ": site_off or win_off does not begin at 0");
    int64_t bound = 0, records = 0, G = 0;
    const int64_t u = in.per_site();
    for (size_t g = 0; g < n; ++g) {
        if (in.site_off[g + 1] < in.site_off[g] || in.site_off[g + 1] - in.site_off[g] > IOC_INSERTS_MAX)
            return ioc_fail(c, IOC_ERR_ARG, who + ": segment " + std::to_string(g) + " has a negative number of sites or more than 32");
        for (int64_t x = in.site_off[g]; x < in.site_off[g + 1]; ++x) {
            if (!in.win || in.win[x].lo < 1 || in.win[x].lo >= in.win[x].hi || in.win[x].hi > ds[g].rlen || in.win[x].tlen < 0)
                return ioc_fail(c, IOC_ERR_ARG, who + ": the window of site " + std::to_string(x) + " does not lie inside its segment");
            if (in.by_variant && (!in.var || (in.var[x].split != 0 && in.var[x].split != 1) || in.var[x].tlen_b < 0))
                return ioc_fail(c, IOC_ERR_ARG, who + ": the variant record of site " + std::to_string(x) + " has a split outside 0 / 1 or a negative tlen_b");
            for (int64_t y = u * x; y < u * (x + 1); ++y)
                if (in.win_off[y + 1] < in.win_off[y]) return ioc_fail(c, IOC_ERR_ARG, who + (in.by_variant ? ": slot_off" : ": win_off") + " does not ascend at site " + std::to_string(x));
        }
        const int64_t most = pile_call_most(ds[g].rlen) + in.room(in.site_off[g], in.site_off[g + 1]);
        if (most > INT32_MAX)  // (the record's out_len, the kernels' byte counts)
            return ioc_fail(c, IOC_ERR_CAPACITY, who + ": an isoform of segment " + std::to_string(g) + " may hold more than 2^31 - 1 bytes");
        bound += int64_t(n_groups[g]) * most, records += int64_t(n_groups[g]) * (in.site_off[g + 1] - in.site_off[g]), G += n_groups[g];
    }
    if (in.win_off[u * in.site_off[n]] > 0 && (!in.wseq || !in.wqual)) return IOC_ERR_ARG;
    if (G > 0 && !in.keys) return IOC_ERR_ARG;
    if (o.cap < records) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": splice_cap " + std::to_string(o.cap) + " below the bound " + std::to_string(records));
    if (records > 0 && !o.splice) return IOC_ERR_ARG;
    *out_bound = bound;
    return call_room_ok(c, who, o.call, bound);
}

// plan -> count -> scan -> write -> copy-out over group tables that lie on the device (g; gseg_off[s] .. gseg_off[s + 1] are segment
// s's group-segments).  a_splice holds, uploaded in one piece, [group-segments][their segments][keys][window records][site_off][win_off]
// [window sequences][window qualities][splice_off][variant records, by variant], and behind them [site records][splice records][plans][plan lengths][seg_len]
// [out_off][records][sequence][qualities].
static int splice_device(SinkRun& r, const GroupPiled& g, const std::vector<uint32_t>& gseg_off, const uint8_t* d_frames, uint64_t frame_bytes, const SpliceIn& in,
                         const SpliceOut& o, int64_t bound)
{
    ioc_ctx* const c = r.c;
    const size_t n = gseg_off.size() - 1, G = g.gsegs.size(), S = size_t(in.site_off[n]), U = size_t(in.per_site()) * S, W = size_t(in.win_off[U]);
    const bool vars = in.by_variant && S > 0;  // (without a site either plan kernel writes the same: nothing)
    std::vector<int32_t> gseg_seg(G);
    o.splice_off[0] = 0;
    for (size_t s = 0; s < n; ++s)
        for (size_t x = gseg_off[s]; x < gseg_off[s + 1]; ++x) gseg_seg[x] = int32_t(s), o.splice_off[x + 1] = o.splice_off[x] + (in.site_off[s + 1] - in.site_off[s]);
    const size_t R = size_t(o.splice_off[G]);
    Arena l;
    const size_t o_gseg = l.take(G * sizeof(IocPileSeg)), o_gs = l.take(G * 4), o_keys = l.take(G * 8), o_win = l.take(S * sizeof(ioc_insert_window)),
                 o_soff = l.take((n + 1) * 8), o_woff = l.take((U + 1) * 8), o_wseq = l.take(W), o_wqual = l.take(W), o_spoff = l.take((G + 1) * 8),
                 o_var = l.take(vars ? S * sizeof(ioc_window_variant) : 0), tables = l.size();
    const size_t o_rec = l.take(R * sizeof(ioc_splice_site)), o_ss = l.take(G * sizeof(ioc_splice_stats)), o_plan = l.take(G * IOC_SPLICE_PLAN_MAX * sizeof(IocSpliceIv)),
                 o_pn = l.take(G * 4), o_len = l.take(G * 8), o_off = l.take((G + 1) * 8), o_st = l.take(G * sizeof(ioc_polish_stats)), o_seq = l.take(size_t(bound)),
                 o_qual = l.take(size_t(bound));
    std::vector<uint8_t> stage(tables, 0);
    auto put = [&](size_t at, const void* src, size_t b) { if (b) memcpy(stage.data() + at, src, b); };
    put(o_gseg, g.gsegs.data(), G * sizeof(IocPileSeg)), put(o_gs, gseg_seg.data(), G * 4), put(o_keys, in.keys, G * 8), put(o_win, in.win, S * sizeof(ioc_insert_window));
    put(o_soff, in.site_off, (n + 1) * 8), put(o_woff, in.win_off, (U + 1) * 8), put(o_wseq, in.wseq, W), put(o_wqual, in.wqual, W), put(o_spoff, o.splice_off, (G + 1) * 8);
    if (vars) put(o_var, in.var, S * sizeof(ioc_window_variant));
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_splice, l.size()));
    uint8_t* p = static_cast<uint8_t*>(c->a_splice.p);
    IOC_CHK(c, hipMemcpyAsync(p, stage.data(), tables, hipMemcpyHostToDevice, c->stream));
    const IocSpliceDev v{reinterpret_cast<const IocPileSeg*>(p + o_gseg), uint32_t(G), reinterpret_cast<const int32_t*>(p + o_gs),
                         reinterpret_cast<const unsigned long long*>(p + o_keys), reinterpret_cast<const ioc_insert_window*>(p + o_win),
                         reinterpret_cast<const long long*>(p + o_soff), reinterpret_cast<const long long*>(p + o_woff), uint64_t(S), p + o_wseq, p + o_wqual, uint64_t(W),
                         reinterpret_cast<const long long*>(p + o_spoff), reinterpret_cast<ioc_splice_site*>(p + o_rec), uint64_t(R),
                         reinterpret_cast<ioc_splice_stats*>(p + o_ss), reinterpret_cast<IocSpliceIv*>(p + o_plan), reinterpret_cast<uint32_t*>(p + o_pn),
                         vars ? reinterpret_cast<const ioc_window_variant*>(p + o_var) : nullptr};
    IOC_TRY(r.begin(r.t.ms_splice[0]));
    IOC_CHK(c, iock_splice_plan(c->stream, v));
    IOC_TRY(r.end());
    IOC_TRY(r.begin(r.t.ms_splice[1]));
    IOC_CHK(c, iock_splice_call(c->stream, v, /*emit*/ false, g.cols, g.ins, uint64_t(g.n_rows), d_frames, frame_bytes, o.call.min_depth, reinterpret_cast<int64_t*>(p + o_len),
                                reinterpret_cast<ioc_polish_stats*>(p + o_st), nullptr, nullptr, nullptr, 0));
    IOC_CHK(c, iock_pile_scan(c->stream, reinterpret_cast<const int64_t*>(p + o_len), uint32_t(G), reinterpret_cast<int64_t*>(p + o_off)));
    IOC_TRY(r.end());
    IOC_TRY(r.begin(r.t.ms_splice[2]));
    IOC_CHK(c, iock_splice_call(c->stream, v, /*emit*/ true, g.cols, g.ins, uint64_t(g.n_rows), d_frames, frame_bytes, o.call.min_depth, nullptr, nullptr,
                                reinterpret_cast<const int64_t*>(p + o_off), p + o_seq, p + o_qual, uint64_t(bound)));
    IOC_TRY(r.end());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    r.settled();
    IOC_TRY(r.copy_out({{o.call.off, p + o_off, (G + 1) * 8}}));
    const int64_t len = o.call.off[G];
    if (len < 0 || len > bound) return ioc_fail(c, IOC_ERR_HIP, "the splice returned a length outside its bound");
    return r.copy_out({{o.call.stats, p + o_st, G * sizeof(ioc_polish_stats)}, {o.sstats, p + o_ss, G * sizeof(ioc_splice_stats)},
                       {o.splice, p + o_rec, R * sizeof(ioc_splice_site)}, {o.call.seq, p + o_seq, size_t(len)}, {o.call.qual, p + o_qual, size_t(len)}});
}

static std::string splice_trace(const AlnTally& t)
{
    char buf[160];
    snprintf(buf, sizeof buf, "k_splice_plan %.3f ms, k_splice_call<count> + scan %.3f ms, k_splice_call<emit> %.3f ms", t.ms_splice[0], t.ms_splice[1], t.ms_splice[2]);
    return buf;
}
}  // namespace

// upload -> groups pile -> splice -> copy-out.  ioc_planes_polish_groups with the windows of the sites every isoform carries spliced
// into its call: the checks of ioc_planes_polish_groups, in its order, then those of the windows.
// `in` says whether the windows are one a site or the variant stage's slots (ioc_planes_isoforms_full_variants).
static int planes_isoforms_full(const std::string& who, const SpliceIn& in, ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                                const int32_t* n_groups, int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* group, const uint8_t* base, const uint8_t* slots,
                                int32_t min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish, ioc_splice_stats* out_sstats,
                                ioc_splice_site* out_splice, int64_t splice_cap, int64_t* splice_off, ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins)
{
    const int64_t* const site_off = in.site_off;
    const SpliceOut o{{min_depth, out_seq, out_qual, cap, out_off, out_polish}, out_sstats, out_splice, splice_cap, splice_off};
    if (!c || n_segs < 0 || n_pairs < 0 || !o.ok() || (n_segs > 0 && (!rlen || !frame_off || !n_groups)) || (n_pairs > 0 && (!seg_of_pair || !group))) return IOC_ERR_ARG;
    SinkPlan p;
    if (int st = p.from_rlen(who, n_segs, rlen, frames, frame_off, n_pairs, seg_of_pair, nullptr, 0)) return ioc_fail(c, st, p.msg);
    if (p.plane_bytes > 0 && (!base || !slots)) return IOC_ERR_ARG;
    int64_t G = 0, bound = 0;
    for (int32_t g = 0; g < n_segs; ++g) {
        if (n_groups[g] < 0) return ioc_fail(c, IOC_ERR_ARG, who + ": segment " + std::to_string(g) + " has a negative number of groups");
        if ((G += n_groups[g]) > INT32_MAX) return ioc_fail(c, IOC_ERR_ARG, who + ": more than 2^31 - 1 group-segments");
    }
    for (int32_t i = 0; i < n_pairs; ++i)
        if (group[i] < -1 || group[i] >= n_groups[seg_of_pair[i]])
            return ioc_fail(c, IOC_ERR_ARG, who + ": the group of pair " + std::to_string(i) + " is neither -1 nor one of its segment's");
    IOC_TRY(splice_ok(c, who, in, o, p.segs, n_groups, &bound));
    out_off[0] = 0, splice_off[0] = 0;
    if (G == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    DevBuf d_frames;
    IOC_TRY(ioc_alloc(c, d_frames, size_t(p.frame_bytes)));
    if (p.frame_bytes > 0) IOC_CHK(c, hipMemcpyAsync(d_frames.p, frames, size_t(p.frame_bytes), hipMemcpyHostToDevice, c->stream));
    SinkRun r{c};
    GroupPiled gp;
    IOC_TRY(r.groups_pile(p, seg_of_pair, group, n_groups, Planes{nullptr, nullptr, nullptr, base, slots}, Planes{}, gp));
    IOC_TRY(splice_device(r, gp, gp.lists.gseg_off, static_cast<const uint8_t*>(d_frames.p), uint64_t(p.frame_bytes), in, o, bound));
    IOC_TRY(r.copy_out({{out_gcols, gp.cols, size_t(gp.n_rows) * sizeof(ioc_pileup_col)}, {out_gins, gp.ins, size_t(gp.n_rows) * sizeof(ioc_pileup_ins)}}));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes isoforms full%s: %lld group-segments, %d pairs, %lld sites, %lld bytes called, k_group_pile %.3f ms, %s\n",
                in.by_variant ? " by variant" : "", (long long)G, n_pairs, (long long)site_off[n_segs], (long long)out_off[G], r.t.ms_group_pile, splice_trace(r.t).c_str());
    return IOC_OK;
}

int ioc_planes_isoforms_full(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, const int32_t* n_groups, int32_t n_pairs,
                             const int32_t* seg_of_pair, const int32_t* group, const uint8_t* base, const uint8_t* slots, const uint64_t* iso_key,
                             const ioc_insert_window* win, const int64_t* site_off, const char* win_seq, const char* win_qual, const int64_t* win_off, int32_t min_depth,
                             char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish, ioc_splice_stats* out_sstats,
                             ioc_splice_site* out_splice, int64_t splice_cap, int64_t* splice_off, ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins)
{
    const SpliceIn in{iso_key, win, site_off, win_seq, win_qual, win_off};
    return planes_isoforms_full("ioc_planes_isoforms_full", in, c, n_segs, rlen, frames, frame_off, n_groups, n_pairs, seg_of_pair, group, base, slots, min_depth, out_seq,
                                out_qual, cap, out_off, out_polish, out_sstats, out_splice, splice_cap, splice_off, out_gcols, out_gins);
}

// ... by variant: the same stages, the plan kernel in its slot-aware instantiation over the slots and the variant records uploaded
// beside the window records.
int ioc_planes_isoforms_full_variants(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, const int32_t* n_groups,
                                      int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* group, const uint8_t* base, const uint8_t* slots,
                                      const uint64_t* iso_key, const ioc_insert_window* win, const ioc_window_variant* var, const int64_t* site_off,
                                      const char* slot_seq, const char* slot_qual, const int64_t* slot_off, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap,
                                      int64_t* out_off, ioc_polish_stats* out_polish, ioc_splice_stats* out_sstats, ioc_splice_site* out_splice, int64_t splice_cap,
                                      int64_t* splice_off, ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins)
{
    const SpliceIn in{iso_key, win, site_off, slot_seq, slot_qual, slot_off, var, /*by_variant*/ true};
    return planes_isoforms_full("ioc_planes_isoforms_full_variants", in, c, n_segs, rlen, frames, frame_off, n_groups, n_pairs, seg_of_pair, group, base, slots, min_depth,
                                out_seq, out_qual, cap, out_off, out_polish, out_sstats, out_splice, splice_cap, splice_off, out_gcols, out_gins);
}

namespace {
// the isoforms of the fused call: how many of a segment are called and where they go (iso_off: n_segs + 1 entries; o.call.off and
// o.splice_off: room for iso_cap + 1 entries)
struct IsoFull {
    int32_t max_iso;
    SpliceOut o;
    int64_t iso_cap;
    int64_t* iso_off;
    bool ok() const { return max_iso >= 1 && o.ok() && iso_cap >= 0 && iso_off; }
};
// what the fused call refuses about its isoforms' room, known before anything runs: a segment has at most min(max_iso, reads)
// isoforms, each at most the call's bound plus min(max_sites, max(rlen - 1, 0)) windows of pile_call_most(max_win) bytes
int iso_full_ok(ioc_ctx* c, const std::string& who, const IsoFull& f, const SinkPlan& p, const std::vector<int64_t>& n_reads, int32_t max_sites, int32_t max_win)
{
    int64_t iso = 0, bytes = 0, records = 0;
    for (size_t g = 0; g < p.segs.size(); ++g) {
        const int64_t k = std::min<int64_t>(f.max_iso, n_reads[g]), sites = std::min<int64_t>(max_sites, std::max<int64_t>(int64_t(p.segs[g].rlen) - 1, 0));
        const int64_t most = pile_call_most(p.segs[g].rlen) + sites * pile_call_most(max_win);
        if (most > INT32_MAX) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": an isoform of segment " + std::to_string(g) + " may hold more than 2^31 - 1 bytes");
        iso += k, bytes += k * most, records += k * sites;
    }
    if (f.iso_cap < iso) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": iso_cap " + std::to_string(f.iso_cap) + " below the bound " + std::to_string(iso));
    if (f.o.cap < records) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": splice_cap " + std::to_string(f.o.cap) + " below the bound " + std::to_string(records));
    if (records > 0 && !f.o.splice) return IOC_ERR_ARG;
    return call_room_ok(c, who, f.o.call, bytes);
}
}  // namespace

// ---- the block family: pile -> blocks -> the stages that are on -> copy-out, one runner behind ten entry points ----
namespace {
struct EndsStage {  // the ends stage behind the block stage, and where the extents the call puts together for it go (a record a pair)
    EndsOut o;
    ioc_read_extent* extents;
};
// What a block-family call is: the alignment, the segments, the block search, and one member per later stage, set where the stage
// is on.  Ten combinations are reachable, an entry point each: none | inserts | ends | inserts windows | inserts windows variants |
// inserts windows full | inserts windows variants full | polish | polish weighted | correct.
struct BlocksCall {
    std::string who;  // the entry point, as its refusals name it
    AlnCall a;
    ioc_aln_stats* out_stats;
    int32_t n_segs;
    const ioc_polish_seg* segs;
    const int32_t* seg_of_pair;
    BlocksOut o;
    ioc_pileup_col* out_cols;
    std::optional<InsertsOut> inserts;
    std::optional<EndsStage> ends;
    std::optional<WindowsOut> windows;     // (behind inserts; its slack and its call's min_depth are the entry point's to set)
    std::optional<VariantsFused> variants;  // (in the window stage's place, which it runs as well)
    std::optional<IsoFull> full;            // (behind windows or variants)
    std::optional<IsoPolish> polish;
    std::optional<IsoCorrectOut> correct;   // (the read correction by isoform, over the block stage's groups)
    // the variant stage's slots as a window call's outputs: the window rule, the slots' room
    WindowsOut variant_windows() const { return WindowsOut{windows->rule, variants->call, windows->win, nullptr, nullptr}; }
};

// what the isoform call behind a block search refuses once its plan is known: a segment has at most as many isoforms as reads
// (every isoform has min_alt >= 1 reads of its own)
static int polish_room_ok(ioc_ctx* c, const std::string& who, const IsoPolish& ip, const SinkPlan& p, const std::vector<int64_t>& reads)
{
    std::vector<int32_t> most(p.segs.size(), 0);
    int64_t iso_bound = 0;
    for (size_t g = 0; g < p.segs.size(); ++g) iso_bound += most[g] = int32_t(std::min<int64_t>(ip.max_iso, reads[g]));
    if (ip.iso_cap < iso_bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": iso_cap " + std::to_string(ip.iso_cap) + " below the bound " + std::to_string(iso_bound));
    return groups_polish_ok(c, who, ip.call, p.segs, most.data());
}

// The room of every stage that is on, in the order the entry points have always refused in: blocks, inserts or ends, windows, the
// variant checks, the full-length isoforms, the isoform call.
static int blocks_call_room_ok(ioc_ctx* c, const BlocksCall& b, const SinkPlan& p, const std::vector<int64_t>& reads)
{
    IOC_TRY(blocks_room_ok(c, b.who, b.o, p));
    if (b.inserts) IOC_TRY(inserts_room_ok(c, b.who, *b.inserts, p));
    if (b.ends) IOC_TRY(ends_room_ok(c, b.who, b.ends->o, p, reads));
    const int64_t sites_most = b.windows ? inserts_bound(p, b.inserts->rule.max_sites) : 0;
    if (b.windows) IOC_TRY(windows_ok(c, b.who, *b.windows, p, nullptr, nullptr, sites_most));
    if (b.variants) {
        const VariantsOut& vo = b.variants->vo;
        if (!vo.rule.ok() || !b.variant_windows().ok() || (b.a.n_pairs > 0 && (!vo.variant || !vo.reads)) || (b.n_segs > 0 && !vo.seg)) return IOC_ERR_ARG;
        IOC_TRY(windows_ok(c, b.who, b.variant_windows(), p, nullptr, nullptr, sites_most, /*slots a site*/ 2));
        if (sites_most > 0 && !vo.var) return IOC_ERR_ARG;
        b.variants->call.off[0] = 0;  // (here, where it has always been set: a call the next check refuses leaves it written)
    }
    if (b.full) IOC_TRY(iso_full_ok(c, b.who, *b.full, p, reads, b.inserts->rule.max_sites, b.windows->rule.max_win));
    if (b.polish) IOC_TRY(polish_room_ok(c, b.who, *b.polish, p, reads));
    if (b.correct) {
        std::vector<uint32_t> q_len(size_t(b.a.n_pairs), 0);
        for (int32_t i = 0; i < b.a.n_pairs; ++i) q_len[size_t(i)] = uint32_t(ioc_seq_len(c, b.a.pairs[i].query));
        IOC_TRY(iso_correct_room_ok(c, b.who, *b.correct, p, b.seg_of_pair, q_len));
    }
    return IOC_OK;
}

// blocks -> inserts: the insert kernels over the planes where they lie, with the block stage's keys and masks where that stage
// left them (its read records and masks stay in a_blocks, the insert stage has a_inserts) and a word per segment from the host
static int blocks_then_inserts(SinkRun& r, const BlocksCall& b, const SinkPlan& p, const PiledDev& d, const BlocksDev& bd, const std::vector<uint64_t>& pre_full)
{
    InsertsPre pre;
    pre.pre_full = pre_full.data();
    if (b.a.n_pairs > 0) {
        static_assert(sizeof(ioc_read_blocks) % 8 == 0 && offsetof(ioc_read_blocks, key) == 0, "a record's first word is its key");
        pre.dev_key = reinterpret_cast<const unsigned long long*>(bd.reads), pre.dev_key_stride = uint32_t(sizeof(ioc_read_blocks) / 8);
        pre.dev_mask = bd.mask, pre.dev_mask_stride = 1;
    }
    return r.inserts(p, b.seg_of_pair, nullptr, nullptr, d.base, d.ilen, pre, *b.inserts);  // (a_inserts is reserved here, after the walks)
}

// blocks -> ends: the extents are put together on the host from the block records and the statistics, both of which the call holds
// there anyway, and uploaded with the stage's tables; pre_group is the block stage's group where that stage left it (a_blocks), the
// ends stage has a_rends
static int blocks_then_ends(SinkRun& r, const BlocksCall& b, const SinkPlan& p, const BlocksDev& bd, const ioc_aln_stats* stats)
{
    const int32_t n_pairs = b.a.n_pairs;
    ioc_read_extent* const ext = b.ends->extents;
    for (int32_t i = 0; i < n_pairs; ++i) ext[i] = ioc_read_extent{b.o.reads[i].first_row, b.o.reads[i].end_row, stats[i].lead_i, stats[i].trail_i};
    static_assert(sizeof(ioc_read_blocks) % 4 == 0 && offsetof(ioc_read_blocks, group) % 4 == 0, "a record's group is a word of its own");
    const int32_t* dev_group = n_pairs > 0 ? reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(bd.reads) + offsetof(ioc_read_blocks, group)) : nullptr;
    return r.ends(p, b.seg_of_pair, ext, nullptr, dev_group, uint32_t(sizeof(ioc_read_blocks) / 4), b.ends->o);
}

// what the variant stage hands back where no site is kept anywhere: key2 is the key and the isoforms counted again are the insert
// stage's, which are on the host already
static void variants_of_no_site(const VariantsOut& vo, const InsertsOut& io, int32_t n_pairs, int32_t n_segs)
{
    for (int32_t i = 0; i < n_pairs; ++i) {
        vo.reads[i] = ioc_read_variants{io.reads[i].key, io.reads[i].group, io.reads[i].how};
        std::fill(vo.variant + size_t(i) * IOC_INSERTS_MAX, vo.variant + (size_t(i) + 1) * IOC_INSERTS_MAX, uint8_t(IOC_WINVAR_NONE));
        if (vo.agree) std::fill(vo.agree + size_t(i) * 2 * IOC_INSERTS_MAX, vo.agree + (size_t(i) + 1) * 2 * IOC_INSERTS_MAX, INT32_MIN);
    }
    for (int32_t g = 0; g < n_segs; ++g) {
        const ioc_inserts_seg& z = io.seg[g];
        vo.seg[g] = ioc_variants_seg{0, 0, z.n_groups, z.n_reads, z.n_direct, z.n_assigned, z.n_rare, z.n_ambiguous};
    }
}

// inserts -> windows, or -> windows and variants: the window kernels over the planes where they lie; the sites and the keys are on
// the host when the insert stage returns and travel back with the tables (32 bytes a site, 8 a pair).  With the variant stage on it
// runs in the window stage's place and returns the window call's outputs as well; the block stage's keys are on the host by then and
// serve as pre_*, a read's mask being both bits of every block its key has a state at.
static int inserts_then_windows(SinkRun& r, const BlocksCall& b, const SinkPlan& p, const PiledDev& d, const std::vector<uint64_t>& pre_full)
{
    ioc_ctx* const c = r.c;
    const int32_t n_pairs = b.a.n_pairs, n_segs = b.n_segs;
    const InsertsOut& io = *b.inserts;
    WindowsReads reads;
    std::vector<uint64_t> keys(size_t(n_pairs), 0);
    for (int32_t i = 0; i < n_pairs; ++i) {
        reads.off.push_back(c->aln_offs[size_t(b.a.pairs[i].query)]), reads.len.push_back(uint32_t(ioc_seq_len(c, b.a.pairs[i].query)));
        keys[size_t(i)] = io.reads[i].key;
    }
    if (!b.variants || io.site_off[n_segs] == 0) {
        if (b.variants) variants_of_no_site(b.variants->vo, io, n_pairs, n_segs);
        return windows_device(r, p, b.seg_of_pair, reads, nullptr, nullptr, d.base, d.qpos, io.sites, io.site_off, keys.data(), *b.windows);
    }
    std::vector<uint64_t> pk(size_t(n_pairs), 0), pm(size_t(n_pairs), 0);
    for (int32_t i = 0; i < n_pairs; ++i)
        pk[size_t(i)] = b.o.reads[i].key, pm[size_t(i)] = blocks_key_mask(b.o.reads[i].key, uint32_t(b.o.seg[b.seg_of_pair[i]].n_blocks));
    IOC_TRY(variants_device(r, p, b.seg_of_pair, reads, nullptr, nullptr, d.base, d.qpos, io.sites, io.site_off, keys.data(), n_pairs > 0 ? pk.data() : nullptr,
                            n_pairs > 0 ? pm.data() : nullptr, n_pairs > 0 ? pre_full.data() : nullptr, b.variant_windows(), b.variants->vo, &b.windows->call));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: window variants: %lld bytes called, %s\n", (long long)b.variants->call.off[2 * io.site_off[n_segs]], variants_trace(r.t).c_str());
    return IOC_OK;
}

// windows -> groups pile over the combined isoforms -> splice: the combined isoforms the insert stage just made, the first
// min(n_groups, max_iso) of a segment — their reads, and the key of the lowest-numbered direct read of each (the records are on the
// host: they are one of the call's outputs) — piled by k_group_pile and spliced.  With the variant stage in the same call the
// isoforms are those it counted again, the keys key2, and the windows its slots.
static int windows_then_full(SinkRun& r, const BlocksCall& b, const SinkPlan& p, const PiledDev& d, const std::vector<int64_t>& n_reads)
{
    ioc_ctx* const c = r.c;
    const size_t n_pairs = size_t(b.a.n_pairs), n_segs = size_t(b.n_segs);
    const IsoFull& full = *b.full;
    const InsertsOut& io = *b.inserts;
    const VariantsFused* const vf = b.variants ? &*b.variants : nullptr;
    std::vector<int32_t> found(n_segs, 0), group(n_pairs, -1);
    std::vector<ioc_read_variants> rd(n_pairs);
    for (size_t g = 0; g < n_segs; ++g) found[g] = vf ? vf->vo.seg[g].n_groups : io.seg[g].n_groups;
    for (size_t i = 0; i < n_pairs; ++i) {
        rd[i] = vf ? vf->vo.reads[i] : ioc_read_variants{io.reads[i].key, io.reads[i].group, io.reads[i].how};
        group[i] = rd[i].group;  // (an isoform behind the cut is in no list: group_member_lists)
    }
    IsoCut cut;
    if (int st = cut.from("insert", n_segs, found.data(), n_reads.data(), full.max_iso, full.iso_off)) return ioc_fail(c, st, cut.msg);
    const int64_t G = full.iso_off[n_segs];
    const std::vector<uint64_t> iso_key = iso_keys(n_pairs, b.seg_of_pair, rd.data(), cut.n_iso.data(), full.iso_off, n_segs);
    if (G > 0) {
        const WindowsOut& wo = *b.windows;
        const SpliceIn in = vf ? SpliceIn{iso_key.data(), wo.win, io.site_off, vf->call.seq, vf->call.qual, vf->call.off, vf->vo.var, /*by_variant*/ true, /*longer_slot_room*/ true}
                               : SpliceIn{iso_key.data(), wo.win, io.site_off, wo.call.seq, wo.call.qual, wo.call.off};
        int64_t bound = 0;
        IOC_TRY(splice_ok(c, b.who, in, full.o, p.segs, cut.n_iso.data(), &bound));
        GroupPiled gp;
        IOC_TRY(r.groups_pile(p, b.seg_of_pair, group.data(), cut.n_iso.data(), Planes{}, Planes{nullptr, nullptr, nullptr, d.base, d.slots}, gp));
        IOC_TRY(splice_device(r, gp, gp.lists.gseg_off, static_cast<const uint8_t*>(c->a_pool.p), uint64_t(c->aln_offs.back()), in, full.o, bound));
    }
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: isoforms full%s: %lld isoforms, %lld bytes called, k_ops_project_ins %.3f ms, k_group_pile over the isoforms %.3f ms, %s\n",
                vf ? " by variant" : "", (long long)G, (long long)full.o.call.off[G], r.t.ms_project_ins, r.t.ms_group_pile, splice_trace(r.t).c_str());
    return IOC_OK;
}

// blocks -> groups pile -> call: the consensus of the first min(n_groups, max_iso) isoforms of every segment, each from its direct
// and assigned reads, with no pair aligned a second time.  The read and segment records are on the host when the block stage
// returns; they say which group-segments there are and who is in them.  weighted: k_group_pile_weighted stands in k_group_pile's
// place over the seven weight planes as well, and the call kernels run in their weighted mode.
static int blocks_then_polish(SinkRun& r, const BlocksCall& b, const SinkPlan& p, const PiledDev& d, const std::vector<int64_t>& n_reads)
{
    ioc_ctx* const c = r.c;
    const size_t n_pairs = size_t(b.a.n_pairs), n_segs = size_t(b.n_segs);
    const IsoPolish& ip = *b.polish;
    std::vector<int32_t> found(n_segs, 0), group(n_pairs, -1);
    for (size_t g = 0; g < n_segs; ++g) found[g] = b.o.seg[g].n_groups;
    for (size_t i = 0; i < n_pairs; ++i) group[i] = b.o.reads[i].group;  // (an isoform behind the cut is in no list: group_member_lists)
    IsoCut cut;
    if (int st = cut.from("block", n_segs, found.data(), n_reads.data(), ip.max_iso, ip.iso_off)) return ioc_fail(c, st, cut.msg);
    if (ip.iso_off[n_segs] == 0) return IOC_OK;
    const uint8_t* const frames = static_cast<const uint8_t*>(c->a_pool.p);
    Planes dev{nullptr, nullptr, nullptr, d.base, d.slots};
    if (!ip.weighted)
        return groups_polish_device(r, GroupPolish{ip.call, nullptr, nullptr}, p, frames, uint64_t(c->aln_offs.back()), b.seg_of_pair, group.data(), cut.n_iso.data(), Planes{}, dev);
    dev.weights = d.weights;
    return groups_polish_weighted_device(r, ip.call, GroupTablesW{nullptr, nullptr, nullptr}, p, frames, uint64_t(c->aln_offs.back()), b.seg_of_pair, group.data(),
                                         cut.n_iso.data(), Planes{}, dev);
}

// blocks -> groups pile -> iso correct: every read held against the tables of its own isoform, the block stage's group, with no pair
// aligned a second time.  The read and segment records are on the host when the block stage returns; the planes — base, slots,
// length, position — lie where the pile projected them, the reads in the pool.
static int blocks_then_correct(SinkRun& r, const BlocksCall& b, const SinkPlan& p, const PiledDev& d)
{
    ioc_ctx* const c = r.c;
    const size_t n_pairs = size_t(b.a.n_pairs), n_segs = size_t(b.n_segs);
    std::vector<int32_t> found(n_segs, 0), group(n_pairs, -1);
    std::vector<uint64_t> q_off(n_pairs, 0);
    std::vector<uint32_t> q_len(n_pairs, 0);
    for (size_t g = 0; g < n_segs; ++g) found[g] = std::max(b.o.seg[g].n_groups, 0);
    for (size_t i = 0; i < n_pairs; ++i) {
        const int32_t h = b.o.reads[i].group;
        group[i] = h >= 0 && h < found[size_t(b.seg_of_pair[i])] ? h : -1;
        q_off[i] = uint64_t(c->aln_offs[size_t(b.a.pairs[i].query)]), q_len[i] = uint32_t(ioc_seq_len(c, b.a.pairs[i].query));
    }
    return r.iso_correct(p, b.seg_of_pair, group.data(), found.data(), static_cast<const uint8_t*>(c->a_pool.p), uint64_t(c->aln_offs.back()), Planes{},
                         Planes{nullptr, nullptr, nullptr, d.base, d.slots}, LongPlanes{}, LongPlanes{d.ilen, d.qpos}, q_off, q_len, *b.correct);
}

// the call's own trace line (the variant and the full-length stages have printed theirs): the tags and the `name X ms` fields are
// what tools/align_*_bench.py read
static void blocks_call_trace(const BlocksCall& b, const SinkPlan& p, const AlnTally& t)
{
    const int32_t n_segs = b.n_segs, n_pairs = b.a.n_pairs;
    const long long rows = (long long)p.n_rows, kept = (long long)b.o.block_off[n_segs];
    const double mb = double(t.copied) * 1e-6;
    const std::string stats = b.out_stats ? ", k_ops_stats " + std::to_string(t.ms_stats) + " ms" : "";
    if (b.windows)
        fprintf(stderr, "[ioc]   aligner: blocks inserts seq: %d segments, %lld rows, %d pairs, %lld blocks kept, %lld sites kept, %lld bytes called, %.3f MB copied from the device in %.3f ms, k_ops_project_ilen %.3f ms, k_ops_project_qpos %.3f ms, ms_blocks %.3f ms, %s, %s\n",
                n_segs, rows, n_pairs, kept, (long long)b.inserts->site_off[n_segs], (long long)b.windows->call.off[b.inserts->site_off[n_segs]], mb, t.ms_copy,
                t.ms_project_ilen, t.ms_project_qpos, t.ms_blocks, inserts_trace(t).c_str(), windows_trace(t).c_str());
    else if (b.inserts)
        fprintf(stderr, "[ioc]   aligner: blocks inserts: %d segments, %lld rows, %d pairs, %lld blocks kept, %lld sites kept, %.3f MB copied from the device in %.3f ms, k_ops_pileup %.3f ms, k_ops_project %.3f ms, k_ops_project_ilen %.3f ms, ms_blocks %.3f ms, %s%s\n",
                n_segs, rows, n_pairs, kept, (long long)b.inserts->site_off[n_segs], mb, t.ms_copy, t.ms_pileup, t.ms_project, t.ms_project_ilen, t.ms_blocks,
                inserts_trace(t).c_str(), stats.c_str());
    else if (b.ends)
        fprintf(stderr, "[ioc]   aligner: blocks ends: %d segments, %lld rows, %d pairs, %lld blocks kept, %lld end sites kept, %lld variants kept, %.3f MB copied from the device in %.3f ms, k_ops_pileup %.3f ms, k_ops_project %.3f ms, ms_blocks %.3f ms, k_ops_stats %.3f ms, %s\n",
                n_segs, rows, n_pairs, kept, (long long)b.ends->o.site_off[2 * n_segs], (long long)b.ends->o.var_off[n_segs], mb, t.ms_copy, t.ms_pileup, t.ms_project,
                t.ms_blocks, t.ms_stats, ends_trace(t).c_str());
    else if (b.polish && b.polish->weighted)
        fprintf(stderr, "[ioc]   aligner: blocks polish weighted: %d segments, %lld rows, %d pairs, %lld blocks kept, %lld isoforms called, %lld bytes called, %.3f MB copied from the device in %.3f ms, k_ops_pileup %.3f ms, k_ops_project %.3f ms, k_ops_project_ins %.3f ms, k_ops_project_weights %.3f ms, ms_blocks %.3f ms, k_group_pile_weighted %.3f ms, k_pile_call<weighted> %.3f ms%s\n",
                n_segs, rows, n_pairs, kept, (long long)b.polish->iso_off[n_segs], (long long)b.polish->call.off[b.polish->iso_off[n_segs]], mb, t.ms_copy, t.ms_pileup,
                t.ms_project, t.ms_project_ins, t.ms_project_weights, t.ms_blocks, t.ms_group_pile_weighted, t.ms_call, stats.c_str());
    else if (b.correct)
        fprintf(stderr, "[ioc]   aligner: blocks correct: %d segments, %lld rows, %d pairs, %lld blocks kept, %lld bytes written, %.3f MB copied from the device in %.3f ms, k_ops_pileup %.3f ms, k_ops_project %.3f ms, k_ops_project_ins %.3f ms, k_ops_project_ilen %.3f ms, k_ops_project_qpos %.3f ms, ms_blocks %.3f ms, k_group_pile %.3f ms, k_iso_correct %.3f ms%s\n",
                n_segs, rows, n_pairs, kept, (long long)b.correct->off[n_pairs], mb, t.ms_copy, t.ms_pileup, t.ms_project, t.ms_project_ins, t.ms_project_ilen, t.ms_project_qpos,
                t.ms_blocks, t.ms_group_pile, t.ms_iso_correct, stats.c_str());
    else if (b.polish)
        fprintf(stderr, "[ioc]   aligner: blocks polish: %d segments, %lld rows, %d pairs, %lld blocks kept, %lld isoforms called, %lld bytes called, %.3f MB copied from the device in %.3f ms, k_ops_pileup %.3f ms, k_ops_project %.3f ms, k_ops_project_ins %.3f ms, ms_blocks %.3f ms, k_group_pile %.3f ms, k_pile_call %.3f ms%s\n",
                n_segs, rows, n_pairs, kept, (long long)b.polish->iso_off[n_segs], (long long)b.polish->call.off[b.polish->iso_off[n_segs]], mb, t.ms_copy, t.ms_pileup,
                t.ms_project, t.ms_project_ins, t.ms_blocks, t.ms_group_pile, t.ms_call, stats.c_str());
    else
        fprintf(stderr, "[ioc]   aligner: blocks: %d segments, %lld rows, %d pairs, %lld blocks kept, %.3f MB (blocks, records%s%s%s) copied from the device in %.3f ms, k_ops_pileup %.3f ms, k_ops_project %.3f ms, ms_blocks %.3f ms%s\n",
                n_segs, rows, n_pairs, kept, mb, b.o.rows ? ", rows" : "", b.out_cols ? ", table" : "", b.out_stats ? ", statistics" : "", t.ms_copy, t.ms_pileup, t.ms_project,
                t.ms_blocks, stats.c_str());
}

// The runner.  ioc_align_pairs_alleles' pile, the table of counts with every pair projected beside it — and with the planes the
// stages that are on read: the length plane for the inserts, the position plane for the windows, the six slot planes for the
// isoforms that are called or spliced, the seven weight planes for the weighted call —, the block kernels over the base planes
// where they lie, and the later stages one behind the other.  What comes back is what each stage made, a record per pair and per
// segment, and the table only where it is asked for.
static int align_pairs_blocks_call(ioc_ctx* c, const BlocksCall& b)
{
    const int32_t n_pairs = b.a.n_pairs, n_segs = b.n_segs;
    if (!c || n_pairs < 0 || n_segs < 0 || !b.o.ok() || (b.inserts && !b.inserts->ok()) || (b.ends && !b.ends->o.ok()) || (b.windows && !b.windows->ok()) ||
        (b.variants && !b.variants->call.off) || (b.full && !b.full->ok()) || (b.polish && !b.polish->ok()) || (b.correct && !b.correct->ok()) ||
        (n_pairs > 0 && (!b.a.pairs || !b.seg_of_pair || (b.ends && !b.ends->extents))) || (n_segs > 0 && !b.segs))
        return IOC_ERR_ARG;
    if (b.polish && b.polish->weighted && !c->aln_qual_set)
        return ioc_fail(c, IOC_ERR_ARG, b.who + ": no qualities are set for the current pool (ioc_align_set_pool_qual)");
    SinkPlan p;
    if (int st = p.from_pool(b.who, c->aln_offs, n_segs, b.segs, n_pairs, b.a.pairs, b.seg_of_pair, 0, PLAN_REFUSE_LONG)) return ioc_fail(c, st, p.msg);
    const std::vector<int64_t> n_reads = reads_per_seg(size_t(n_segs), size_t(n_pairs), b.seg_of_pair);
    IOC_TRY(blocks_call_room_ok(c, b, p, n_reads));

    for (int32_t i = 0; i < n_pairs && b.out_stats; ++i) b.out_stats[i] = ioc_aln_stats{};
    for (int32_t i = 0; i < n_pairs && b.ends; ++i) b.ends->extents[i] = ioc_read_extent{0, 0, 0, 0};
    b.o.block_off[0] = 0;
    if (b.inserts) b.inserts->site_off[0] = 0;
    if (b.ends) b.ends->o.site_off[0] = 0, b.ends->o.var_off[0] = 0;
    if (b.windows) b.windows->call.off[0] = 0;
    if (b.full) b.full->o.call.off[0] = 0, b.full->o.splice_off[0] = 0;
    if (b.polish) b.polish->call.off[0] = 0;
    if (b.correct) b.correct->off[0] = 0;
    for (int32_t g = 0; g <= n_segs && b.full; ++g) b.full->iso_off[g] = 0;
    for (int32_t g = 0; g <= n_segs && b.polish; ++g) b.polish->iso_off[g] = 0;
    if (n_segs == 0) return b.a.run(c, nullptr);

    // (the ends stage reads every pair's statistics: the statistics kernel runs for it, into the call's own records where none are asked)
    std::vector<ioc_aln_stats> own_stats(b.ends && !b.out_stats ? size_t(n_pairs) : 0, ioc_aln_stats{});
    ioc_aln_stats* const stats = b.ends && !b.out_stats ? own_stats.data() : b.out_stats;
    SinkRun r{c};
    PiledDev d;
    BlocksDev bd{};
    IOC_TRY(r.pile(b.a, PileKind::counts, stats, p.row_base.data(), p.n_rows, p.plane.data(), p.plane_bytes,
                   PileProject{/*ins*/ b.full || b.polish || b.correct, /*weights*/ b.polish && b.polish->weighted, /*ilen*/ b.inserts || b.correct,
                               /*qpos*/ b.windows || b.correct},
                   d));
    IOC_TRY(r.blocks(p, b.seg_of_pair, nullptr, d.base, b.o, &bd));  // (a_blocks is reserved here, after the walks; the records are the host's from here on)
    const auto cols_out = [&] { return r.copy_out({{b.out_cols, d.cols, size_t(p.n_rows) * sizeof(ioc_pileup_col)}}); };
    if (b.inserts) {
        const std::vector<uint64_t> pre_full = blocks_pre_full(size_t(n_segs), b.o.seg);
        IOC_TRY(blocks_then_inserts(r, b, p, d, bd, pre_full));
        if (b.windows) {
            IOC_TRY(cols_out());  // (before the window call: a_pile is the call stage's to take)
            IOC_TRY(inserts_then_windows(r, b, p, d, pre_full));
        }
        if (b.full) IOC_TRY(windows_then_full(r, b, p, d, n_reads));
    }
    if (b.ends) IOC_TRY(blocks_then_ends(r, b, p, bd, stats));
    if (b.polish) IOC_TRY(blocks_then_polish(r, b, p, d, n_reads));
    if (b.correct) IOC_TRY(blocks_then_correct(r, b, p, d));
    if (!b.windows) IOC_TRY(cols_out());
    if (getenv("IOC_TRACE")) blocks_call_trace(b, p, r.t);
    return IOC_OK;
}
}  // namespace

// The ten entry points: each packs its arguments into the record and runs it.
// pile -> blocks -> copy-out
int ioc_align_pairs_blocks(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                           int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs,
                           const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t min_block,
                           int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off,
                           ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols)
{
    const BlocksCall b{"ioc_align_pairs_blocks", {n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs, seg_of_pair,
                       {{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg}, out_cols};
    return align_pairs_blocks_call(c, b);
}

// pile -> blocks -> inserts -> copy-out: the length plane projected beside the two, and the insert kernels behind the block kernels
int ioc_align_pairs_blocks_inserts(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                   int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                   const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                                   int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap,
                                   int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t min_ins,
                                   int32_t slack, int32_t max_sites, ioc_insert_row* out_irows, ioc_pile_insert* out_sites, int64_t sites_cap,
                                   int64_t* site_off, ioc_read_inserts* out_ireads, ioc_inserts_seg* out_iseg)
{
    BlocksCall b{"ioc_align_pairs_blocks_inserts", {n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs, seg_of_pair,
                 {{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg}, out_cols};
    b.inserts = InsertsOut{{min_ins, slack, min_depth, min_alt, min_pct, max_sites}, out_irows, out_sites, sites_cap, site_off, out_ireads, out_iseg};
    return align_pairs_blocks_call(c, b);
}

// pile -> blocks -> ends -> copy-out: the statistics kernel run over every slice, and the ends kernels behind the block kernels
int ioc_align_pairs_blocks_ends(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs,
                                const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t min_block,
                                int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off,
                                ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t slack, int32_t min_over,
                                int32_t ends_min_pct, int32_t max_sites, int32_t max_variants, ioc_read_extent* out_extents, ioc_end_row* out_erows,
                                ioc_end_site* out_sites, int64_t sites_cap, int64_t* site_off, ioc_end_variant* out_variants, int64_t variants_cap,
                                int64_t* var_off, ioc_read_ends* out_ereads, ioc_ends_seg* out_eseg)
{
    BlocksCall b{"ioc_align_pairs_blocks_ends", {n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs, seg_of_pair,
                 {{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg}, out_cols};
    b.ends = EndsStage{{{slack, min_over, min_depth, min_alt, ends_min_pct, max_sites, max_variants}, out_erows, out_sites, sites_cap, site_off, out_variants, variants_cap,
                        var_off, out_ereads, out_eseg}, out_extents};
    return align_pairs_blocks_call(c, b);
}

// pile -> blocks -> inserts -> windows -> copy-out: the position plane projected beside the other two, and the window kernels behind
// the insert kernels
int ioc_align_pairs_blocks_inserts_seq(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                       int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                       const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                                       int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap,
                                       int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t min_ins,
                                       int32_t slack, int32_t max_sites, ioc_insert_row* out_irows, ioc_pile_insert* out_sites, int64_t sites_cap,
                                       int64_t* site_off, ioc_read_inserts* out_ireads, ioc_inserts_seg* out_iseg, int32_t max_win, int32_t win_match,
                                       int32_t win_mismatch, int32_t win_gap, int32_t polish_min_depth, ioc_insert_window* out_win, char* out_wseq, char* out_wqual,
                                       int64_t win_cap, int64_t* out_woff, ioc_polish_stats* out_wstats)
{
    BlocksCall b{"ioc_align_pairs_blocks_inserts_seq", {n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs, seg_of_pair,
                 {{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg}, out_cols};
    b.inserts = InsertsOut{{min_ins, slack, min_depth, min_alt, min_pct, max_sites}, out_irows, out_sites, sites_cap, site_off, out_ireads, out_iseg};
    b.windows = WindowsOut{{slack, max_win, win_match, win_mismatch, win_gap}, {polish_min_depth, out_wseq, out_wqual, win_cap, out_woff, out_wstats}, out_win, nullptr, nullptr};
    return align_pairs_blocks_call(c, b);
}

// ... -> inserts -> windows and variants -> copy-out: the variant kernels behind the window kernels, over the planes where they lie
int ioc_align_pairs_blocks_inserts_variants(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                            int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                            const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                                            int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap,
                                            int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t min_ins,
                                            int32_t slack, int32_t max_sites, ioc_insert_row* out_irows, ioc_pile_insert* out_sites, int64_t sites_cap,
                                            int64_t* site_off, ioc_read_inserts* out_ireads, ioc_inserts_seg* out_iseg, int32_t max_win, int32_t win_match,
                                            int32_t win_mismatch, int32_t win_gap, int32_t polish_min_depth, ioc_insert_window* out_win, char* out_wseq, char* out_wqual,
                                            int64_t win_cap, int64_t* out_woff, ioc_polish_stats* out_wstats, int32_t min_agree, ioc_window_variant* out_var,
                                            char* out_vseq, char* out_vqual, int64_t var_cap, int64_t* out_voff, ioc_polish_stats* out_vstats, uint8_t* out_variant,
                                            int32_t* out_agree, ioc_read_variants* out_vreads, ioc_variants_seg* out_vseg)
{
    BlocksCall b{"ioc_align_pairs_blocks_inserts_variants", {n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs, seg_of_pair,
                 {{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg}, out_cols};
    b.inserts = InsertsOut{{min_ins, slack, min_depth, min_alt, min_pct, max_sites}, out_irows, out_sites, sites_cap, site_off, out_ireads, out_iseg};
    b.windows = WindowsOut{{slack, max_win, win_match, win_mismatch, win_gap}, {polish_min_depth, out_wseq, out_wqual, win_cap, out_woff, out_wstats}, out_win, nullptr, nullptr};
    b.variants = VariantsFused{{{min_agree, min_alt, min_pct}, out_var, out_variant, out_agree, out_vreads, out_vseg}, {polish_min_depth, out_vseq, out_vqual, var_cap, out_voff, out_vstats}};
    return align_pairs_blocks_call(c, b);
}

// ... -> windows -> groups pile over the combined isoforms -> splice -> copy-out: the six slot planes projected as well (13 bytes per
// row and pair), and behind the window kernels k_group_pile over the combined isoforms and the splice kernels
int ioc_align_pairs_isoforms_full(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                  int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                  const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                                  int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap,
                                  int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t min_ins,
                                  int32_t slack, int32_t max_sites, ioc_insert_row* out_irows, ioc_pile_insert* out_sites, int64_t sites_cap,
                                  int64_t* site_off, ioc_read_inserts* out_ireads, ioc_inserts_seg* out_iseg, int32_t max_win, int32_t win_match,
                                  int32_t win_mismatch, int32_t win_gap, int32_t polish_min_depth, ioc_insert_window* out_win, char* out_wseq, char* out_wqual,
                                  int64_t win_cap, int64_t* out_woff, ioc_polish_stats* out_wstats, int32_t max_iso, char* out_seq, char* out_qual, int64_t cap,
                                  int64_t* out_off, ioc_polish_stats* out_polish, ioc_splice_stats* out_sstats, ioc_splice_site* out_splice, int64_t splice_cap,
                                  int64_t* splice_off, int64_t iso_cap, int64_t* iso_off)
{
    BlocksCall b{"ioc_align_pairs_isoforms_full", {n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs, seg_of_pair,
                 {{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg}, out_cols};
    b.inserts = InsertsOut{{min_ins, slack, min_depth, min_alt, min_pct, max_sites}, out_irows, out_sites, sites_cap, site_off, out_ireads, out_iseg};
    b.windows = WindowsOut{{slack, max_win, win_match, win_mismatch, win_gap}, {polish_min_depth, out_wseq, out_wqual, win_cap, out_woff, out_wstats}, out_win, nullptr, nullptr};
    b.full = IsoFull{max_iso, {{polish_min_depth, out_seq, out_qual, cap, out_off, out_polish}, out_sstats, out_splice, splice_cap, splice_off}, iso_cap, iso_off};
    return align_pairs_blocks_call(c, b);
}

// ... -> windows and variants -> groups pile over the isoforms counted again -> splice by variant -> copy-out.  The two calls above in
// one: the variant stage's key2, groups and slots feed the splice where the insert stage's keys, groups and windows did.
int ioc_align_pairs_isoforms_full_variants(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                           int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                           const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                                           int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap,
                                           int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t min_ins,
                                           int32_t slack, int32_t max_sites, ioc_insert_row* out_irows, ioc_pile_insert* out_sites, int64_t sites_cap,
                                           int64_t* site_off, ioc_read_inserts* out_ireads, ioc_inserts_seg* out_iseg, int32_t max_win, int32_t win_match,
                                           int32_t win_mismatch, int32_t win_gap, int32_t polish_min_depth, ioc_insert_window* out_win, char* out_wseq, char* out_wqual,
                                           int64_t win_cap, int64_t* out_woff, ioc_polish_stats* out_wstats, int32_t min_agree, ioc_window_variant* out_var,
                                           char* out_vseq, char* out_vqual, int64_t var_cap, int64_t* out_voff, ioc_polish_stats* out_vstats, uint8_t* out_variant,
                                           int32_t* out_agree, ioc_read_variants* out_vreads, ioc_variants_seg* out_vseg, int32_t max_iso, char* out_seq, char* out_qual,
                                           int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish, ioc_splice_stats* out_sstats, ioc_splice_site* out_splice,
                                           int64_t splice_cap, int64_t* splice_off, int64_t iso_cap, int64_t* iso_off)
{
    BlocksCall b{"ioc_align_pairs_isoforms_full_variants", {n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs, seg_of_pair,
                 {{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg}, out_cols};
    b.inserts = InsertsOut{{min_ins, slack, min_depth, min_alt, min_pct, max_sites}, out_irows, out_sites, sites_cap, site_off, out_ireads, out_iseg};
    b.windows = WindowsOut{{slack, max_win, win_match, win_mismatch, win_gap}, {polish_min_depth, out_wseq, out_wqual, win_cap, out_woff, out_wstats}, out_win, nullptr, nullptr};
    b.variants = VariantsFused{{{min_agree, min_alt, min_pct}, out_var, out_variant, out_agree, out_vreads, out_vseg}, {polish_min_depth, out_vseq, out_vqual, var_cap, out_voff, out_vstats}};
    b.full = IsoFull{max_iso, {{polish_min_depth, out_seq, out_qual, cap, out_off, out_polish}, out_sstats, out_splice, splice_cap, splice_off}, iso_cap, iso_off};
    return align_pairs_blocks_call(c, b);
}

// pile -> blocks -> groups pile -> call -> copy-out: the six slot planes projected beside the two, and behind the block kernels
// k_group_pile and the call kernels over the planes
int ioc_align_pairs_blocks_polish(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                  int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                  const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                                  int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap,
                                  int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t max_iso,
                                  int32_t polish_min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish,
                                  int64_t iso_cap, int64_t* iso_off)
{
    BlocksCall b{"ioc_align_pairs_blocks_polish", {n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs, seg_of_pair,
                 {{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg}, out_cols};
    b.polish = IsoPolish{max_iso, {polish_min_depth, out_seq, out_qual, cap, out_off, out_polish}, iso_cap, iso_off};
    return align_pairs_blocks_call(c, b);
}

// pile -> blocks -> weighted groups pile -> weighted call -> copy-out: ioc_align_pairs_blocks_polish with every isoform called by
// weight — the pile projects the seven weight planes as well (k_ops_project_weights, under the pool's qualities)
int ioc_align_pairs_blocks_polish_weighted(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                           int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                           const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth, int32_t min_alt,
                                           int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks,
                                           int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols,
                                           int32_t max_iso, int32_t polish_min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off,
                                           ioc_polish_stats* out_polish, int64_t iso_cap, int64_t* iso_off)
{
    BlocksCall b{"ioc_align_pairs_blocks_polish_weighted", {n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs, seg_of_pair,
                 {{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg}, out_cols};
    b.polish = IsoPolish{max_iso, {polish_min_depth, out_seq, out_qual, cap, out_off, out_polish}, iso_cap, iso_off, /*weighted*/ true};
    return align_pairs_blocks_call(c, b);
}

// pile -> blocks -> groups pile -> iso correct -> copy-out: the slot, length and position planes projected beside the base plane, and
// every read corrected against the tables of its own isoform behind the block kernels
int ioc_align_pairs_blocks_correct(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                   int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                   const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                                   int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap,
                                   int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t correct_min_depth,
                                   int32_t correct_min_alt, int32_t correct_min_pct, int32_t correct_max_run, char* out_seq, char* out_qual, int64_t cap,
                                   int64_t* out_off, ioc_iso_correct_stats* out_correct)
{
    BlocksCall b{"ioc_align_pairs_blocks_correct", {n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs, seg_of_pair,
                 {{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks}, out_rows, out_blocks, blocks_cap, block_off, out_reads, out_seg}, out_cols};
    b.correct = IsoCorrectOut{{correct_min_depth, correct_min_alt, correct_min_pct, correct_max_run}, out_seq, out_qual, cap, out_off, out_correct};
    return align_pairs_blocks_call(c, b);
}

// upload -> split.  The split of segments whose sites and alleles the caller holds: both are uploaded, and the kernels run as
// behind ioc_align_pairs_split.
int ioc_alleles_split(ioc_ctx* c, int32_t n_segs, int32_t n_pairs, const int32_t* seg_of_pair, const ioc_pile_site* sites, const int64_t* site_off,
                      const uint8_t* alleles, const int64_t* allele_off, int32_t min_link, int32_t min_margin, int32_t rounds, int64_t* out_link,
                      int8_t* out_phase, uint8_t* out_group, int32_t* out_vote, ioc_split_seg* out_seg)
{
    const SplitCall sp{min_link, min_margin, rounds, out_link, out_phase, out_group, out_vote, out_seg};
    if (!c || n_segs < 0 || n_pairs < 0 || !sp.ok() || (n_segs > 0 && (!site_off || !out_seg)) || (n_pairs > 0 && (!seg_of_pair || !allele_off || !out_group)))
        return IOC_ERR_ARG;
    if (n_segs > 0 && site_off[0] != 0) return ioc_fail(c, IOC_ERR_ARG, "ioc_alleles_split: site_off does not start at 0");
    for (int32_t g = 0; g < n_segs; ++g)
        if (site_off[g + 1] < site_off[g] || site_off[g + 1] - site_off[g] > INT32_MAX)
            return ioc_fail(c, IOC_ERR_ARG, "ioc_alleles_split: site_off descends or segment " + std::to_string(g) + " has more than 2^31 - 1 sites");
    if (n_pairs > 0 && allele_off[0] != 0) return ioc_fail(c, IOC_ERR_ARG, "ioc_alleles_split: allele_off does not start at 0");
    for (int32_t i = 0; i < n_pairs; ++i) {
        if (seg_of_pair[i] < 0 || seg_of_pair[i] >= n_segs) return ioc_fail(c, IOC_ERR_ARG, "ioc_alleles_split: pair " + std::to_string(i) + " names no segment");
        if (allele_off[i + 1] - allele_off[i] != site_off[seg_of_pair[i] + 1] - site_off[seg_of_pair[i]])
            return ioc_fail(c, IOC_ERR_ARG, "ioc_alleles_split: the alleles of pair " + std::to_string(i) + " are not one byte per site of its segment");
    }
    if ((n_segs > 0 && site_off[n_segs] > 0 && !sites) || (n_pairs > 0 && allele_off[n_pairs] > 0 && !alleles)) return IOC_ERR_ARG;
    if (n_segs == 0) return IOC_OK;
    SinkRun r{c};
    Planes laid{};
    IOC_TRY(r.split(sp, size_t(n_segs), size_t(n_pairs), seg_of_pair, site_off, allele_off, sites, alleles, false, laid));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   split: %d segments, %d pairs, %lld sites, %lld allele bytes, %s\n", n_segs, n_pairs, (long long)site_off[n_segs],
                (long long)(n_pairs ? allele_off[n_pairs] : 0), split_trace(r.t).c_str());
    return IOC_OK;
}

int ioc_pileup_call(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, const ioc_pileup_col* cols,
                    const ioc_pileup_ins* ins, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_stats)
{
    return pileup_call_tables(c, n_segs, rlen, frames, frame_off, cols, nullptr, ins, CallOut{min_depth, out_seq, out_qual, cap, out_off, out_stats});
}

int ioc_pileup_call_weighted(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                             const ioc_pileup_col* cols, const ioc_pileup_col* wcols, const ioc_pileup_ins* wins, int32_t min_depth, char* out_seq, char* out_qual, int64_t
                             cap, int64_t* out_off, ioc_polish_stats* out_stats)
{
    if (n_segs > 0 && !wcols) return IOC_ERR_ARG;
    return pileup_call_tables(c, n_segs, rlen, frames, frame_off, cols, wcols, wins, CallOut{min_depth, out_seq, out_qual, cap, out_off, out_stats});
}

int ioc_align_pairs_polish(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                           int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                           const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap,
                           int64_t* out_off, ioc_polish_stats* out_polish, ioc_pileup_col* out_cols, ioc_pileup_ins* out_ins)
{
    return align_pairs_polish(c, AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs,
                              seg_of_pair, CallOut{min_depth, out_seq, out_qual, cap, out_off, out_polish}, out_cols, out_ins, false, nullptr);
}

int ioc_align_pairs_polish_weighted(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t
                                    gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                    const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, char* out_seq, char* out_qual, int64_t
                                    cap, int64_t* out_off, ioc_polish_stats* out_polish, ioc_pileup_col* out_cols, ioc_pileup_col* out_wcols,
                                    ioc_pileup_ins* out_wins)
{
    return align_pairs_polish(c, AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs,
                              seg_of_pair, CallOut{min_depth, out_seq, out_qual, cap, out_off, out_polish}, out_cols, out_wins, true, out_wcols);
}

}  // extern "C"
