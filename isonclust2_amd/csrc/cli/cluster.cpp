// cluster  (src/main.cpp:238-382 + the bookkeeping of src/cluster.cpp:67-322), as stages over one ClusterJob
#include <getopt.h>
#include <unistd.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <future>
#include <iostream>
#include <map>
#include <tuple>
#include <vector>

#include "common.hpp"

using namespace cer;
using std::cerr;
using std::endl;
using std::string;

namespace {

typedef std::chrono::steady_clock Clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

struct ClusterOptions {
    string left_path, right_path, out_path;
    int mode = None, min_cls = -1;
    int spoa_algo = IOC_POA_LOCAL;  // (the reference's code default is 2, semi-global: DESIGN.md §9)
    bool min_purge = false, keep_seq = false;
};

// The right batch as the device path takes it.  Owns its arrays: `view` points into them.
struct RightView {
    std::vector<int64_t> of, orv, roff;
    std::vector<uint32_t> raw_len, hpc_len;
    std::vector<double> score, raw_err, hpc_err;
    std::vector<uint8_t> state;
    std::vector<int32_t> nmem;
    std::shared_ptr<void> mv_mem, mp_mem, rseq_mem;  // (huge pages: 191 MB of first touches on config 2's batch)
    ioc_batch_view view{};
};

// The left batch in the same way: the representatives' error rates and sequences, the MinDB as keys, offsets and postings.
struct LeftView {
    std::vector<double> hpc_err, raw_err;
    std::vector<int64_t> off, k_offs;
    std::vector<uint32_t> keys, post;
    string seq;
    ioc_left_view view{};
};

// consensus mode: a representative replaced by a consensus, written into its cluster after the member moves
struct RepEvent {
    int32_t entry = -1;
    string raw, hpc;
    char qual = '!';
    double raw_err = 0, raw_score = 0, hpc_err = 0;
    std::vector<Minimizer> mins, rev;
};

// consensus mode: the graphs live in this build's POA engine (spoa is not in the reference tree)
struct ConsensusSession {
    ioc_poa* poa = nullptr;
    ioc_consensus_ops ops{};
    std::map<int32_t, RepEvent> rep_events;  // last event per cluster
    ~ConsensusSession()  // (a served job that leaves through die() must not leave its engine behind)
    {
        if (poa && g_served) ioc_poa_destroy(poa);
    }
};

// What each stage leaves for the next.  Everything lives until main_cluster returns (served) or the process leaves (one-shot):
// giving a gigabyte of views back earlier would put its munmap into the one-shot path.
struct ClusterJob {
    ClusterOptions opt;
    Clock::time_point t_begin, t_core;
    std::future<std::pair<ioc_ctx*, double>> ctx_future;  // context creation and prewarm, beside the loads and the flattenings
    Batch left, right;
    std::future<void> unlink_old;  // the old output's pages given back beside the GPU's start; awaited before the save
    bool cons_on = false;          // consensus mode: frozen at sort time (-c), cluster.cpp:101
    bool need_seq = false;
    int n = 0, L = 0;  // entries of the right batch, clusters of the left batch before the moves
    RightView rv;
    LeftView lv;
    ioc_ctx* c = nullptr;
    std::vector<int32_t> out_cls;
    std::vector<int8_t> out_strand;
    ioc_cluster_stats st{};
    ConsensusSession cons;
    double load_ms = 0, flatten_ms = 0, ctx_ms = 0, core_ms = 0, trim_ms = 0, book_ms = 0, save_ms = 0;
};

ClusterOptions parse_cluster_options(int argc, char** argv)
{
    static const struct option lo[] = {
        {"quiet", no_argument, 0, 'Q'}, {"version", no_argument, 0, 'V'}, {"verbose", no_argument, 0, 'v'},
        {"min-purge", no_argument, 0, 'z'}, {"min-cls-size", required_argument, 0, 'F'}, {"keep-seq", no_argument, 0, 'j'},
        {"debug", no_argument, 0, 'd'}, {"spoa-algo", required_argument, 0, 'A'}, {"mode", required_argument, 0, 'x'},
        {"help", no_argument, 0, 'h'}, {"outfile", required_argument, 0, 'o'}, {"left-batch", required_argument, 0, 'l'},
        {"right-batch", required_argument, 0, 'r'}, {0, 0, 0, 0}};
    ClusterOptions opt;
    int o;
    while ((o = getopt_long(argc, argv, "Vdhvo:l:r:Qx:A:zjF:", lo, nullptr)) != -1) {
        switch (o) {
            case 'o': opt.out_path = optarg; break;
            case 'l': opt.left_path = optarg; break;
            case 'r': opt.right_path = optarg; break;
            case 'v': VERBOSE = true; break;
            case 'z': opt.min_purge = true; break;
            case 'j': opt.keep_seq = true; break;
            case 'F': opt.min_cls = atoi(optarg); break;
            case 'x': opt.mode = parse_mode(optarg); break;
            case 'A': opt.spoa_algo = atoi(optarg); break;
            case 'h':
                cerr << "isONclust2-hip cluster -l left.cer [-r right.cer] -o out.cer [-x fast|sahlin|furious] [-A 0|1|2] [-F n] [-z] [-j] [-v]" << endl
                     << "\t-A --spoa-algo  consensus alignment: 0 local (the default here; the reference's code defaults to 2), 1 global, 2 semi-global" << endl;
                exit(0);
            default: break;
        }
    }
    if (opt.left_path.empty()) die("Specifying left input batch is mandatory!");
    if (opt.out_path.empty()) die("Specifying output batch file is mandatory!");
    return opt;
}

// HIP initialisation (~80 ms) runs beside the archive load
std::pair<ioc_ctx*, double> start_context()
{
    const auto t0 = Clock::now();
    const bool fresh = g_srv_ctx == nullptr;
    ioc_ctx* cc = g_srv_ctx ? g_srv_ctx : make_ctx();
    if (g_served) g_srv_ctx = cc;
    if (fresh && !getenv("IOC_NO_PREWARM")) (void)ioc_ctx_prewarm(cc, 1);  // (code objects load beside the flattening and the uploads)
    return std::make_pair(cc, ms_since(t0));
}

// Both archives (a single input becomes the right batch of an empty left one), the start of the old output's removal, and the
// batch compatibility checks
void load_inputs(ClusterJob& job)
{
    const ClusterOptions& opt = job.opt;
    Batch &left = job.left, &right = job.right;
    string err;
    if (!load_batch(left, opt.left_path, err)) die(err);
    job.load_ms = ms_since(job.t_begin);
    if (VERBOSE) {
        cerr << "Loaded input batch from " << opt.left_path << ":" << endl;
        print_batch_info(left);
    }
    if (!opt.right_path.empty()) {
        if (!load_batch(right, opt.right_path, err)) die(err);
        job.load_ms = ms_since(job.t_begin);
        cerr << "Loaded input batch from " << opt.right_path << ":" << endl;
        right.Db.clear();
        print_batch_info(right);
    } else {  // CreatePseudoBatch, serialize.cpp:29-43
        right.BatchNr = -left.BatchNr;
        right.BatchStart = left.BatchStart;
        right.BatchEnd = left.BatchEnd;
        right.BatchBases = 0;
        right.SortArgs = left.SortArgs;
        right.Depth = -1;
        right.Cls = left.Cls;
        right.NrCls = int32_t(right.Cls.size());
        left.Cls.clear();
        if (left.Depth > 0) left.Depth = -left.Depth;
        left.NrCls = 0;
        left.Db.clear();
    }
    // An output file that exists is going to be replaced: giving its pages back (50 - 90 ms for a 460 MB file in the page cache,
    // which O_TRUNC would spend between the last kernel and the first byte written) happens now, beside the GPU's start.  After
    // the loads: the output may be one of the inputs, whose mapping keeps the old file alive.
    job.unlink_old = std::async(std::launch::async, [out_path = opt.out_path] { (void)unlink(out_path.c_str()); });
    left.SortArgs.Mode = opt.mode;
    right.SortArgs.Mode = opt.mode;
    if (opt.min_cls > 0) left.SortArgs.MinClsSize = opt.min_cls;
    if (VERBOSE && opt.mode == None) die("Invalid clustering mode: 3");
    // ---- batch compatibility checks, cluster.cpp:70-90 ----
    const CmdArgs &x = left.SortArgs, &y = right.SortArgs;
    if (!(x.KmerSize == y.KmerSize && x.WindowSize == y.WindowSize && x.MinShared == y.MinShared && x.MinQual == y.MinQual &&
          x.MappedThreshold == y.MappedThreshold && x.AlignedThreshold == y.AlignedThreshold &&
          x.MinFraction == y.MinFraction && x.MinProbNoHits == y.MinProbNoHits && x.Mode == y.Mode))
        die("The left and right batches have been sorted with different parameters! \nRefusing to carry on with clustering as results would not make sense! ");
    if (right.Depth > 0 && right.BatchStart != left.BatchEnd + 1) die("Trying to merge non-consecutive batches! Giving up!");
    if (left.Depth > 0 && right.Depth > left.Depth) die("The left input batch must have higher depth!");
    job.cons_on = left.SortArgs.ConsMaxSize > 0;
    job.need_seq = job.cons_on || opt.mode == Sahlin || opt.mode == Furious;
    job.n = int(right.Cls.size());
    job.L = int(left.Cls.size());
}

// the representative of entry i of the right batch, nullptr for a placeholder
ProcSeq* rep_of(const Batch& right, int i)
{
    auto& e = right.Cls[size_t(i)];
    if (!e || e->empty() || !e->at(0) || !e->at(0)->RawSeq) return nullptr;
    return e->at(0).get();
}

// AoS (Min, Pos, Index) -> SoA, entries spread over the host cores
void minimizers_to_soa(const Batch& right, const RightView& v, uint32_t* mv, uint32_t* mp)
{
    const int n = int(right.Cls.size());
    const unsigned nt = host_threads(16);
    std::atomic<int> bad(0);
    run_threads(nt, [&](unsigned t0) {
        for (int i = int(t0); i < n; i += int(nt)) {
            ProcSeq* r = rep_of(right, i);
            if (!r) continue;
            unsigned wrong = 0;
            auto side = [&](const Span<Minimizer>& mins, int64_t at) {
                uint32_t* val = mv + at;
                uint32_t* pos = mp + at;
                const Minimizer* m = mins.data();  // (packed: read where the archive has them)
                for (size_t t = 0, e = mins.size(); t < e; ++t) {
                    wrong |= m[t].Index ^ uint32_t(t);
                    val[t] = m[t].Min;
                    pos[t] = m[t].Pos;
                }
            };
            side(r->Mins, v.of[size_t(i)]);
            side(r->RevMins, v.orv[size_t(i)]);
            if (wrong) bad = 1;
        }
    });
    if (bad) die("Minimizer Index is not the ordinal");
}

// ---- right batch -> ioc_batch_view ----
void flatten_right(const Batch& right, bool need_seq, const CmdArgs& a, RightView& v)
{
    const int n = int(right.Cls.size());
    const size_t n1 = static_cast<size_t>(n) + 1;
    v.of.assign(n1, 0), v.orv.assign(n1, 0), v.roff.assign(n1, 0);
    v.raw_len.assign(n1, 0), v.hpc_len.assign(n1, 0);
    v.score.assign(n1, -1.0), v.raw_err.assign(n1, 1.0), v.hpc_err.assign(n1, 1.0);
    v.state.assign(n1, 1);
    v.nmem.assign(n1, 0);
    int64_t tot = 0, rtot = 0;
    for (int i = 0; i < n; ++i) {
        v.of[size_t(i)] = tot;
        if (ProcSeq* r = rep_of(right, i)) tot += int64_t(r->Mins.size());
    }
    v.of[size_t(n)] = tot;
    for (int i = 0; i < n; ++i) {
        v.orv[size_t(i)] = tot;
        if (ProcSeq* r = rep_of(right, i)) tot += int64_t(r->RevMins.size());
    }
    v.orv[size_t(n)] = tot;
    v.mv_mem = huge_alloc((static_cast<size_t>(tot) + 1) * 4), v.mp_mem = huge_alloc((static_cast<size_t>(tot) + 1) * 4);
    uint32_t* const mv = static_cast<uint32_t*>(v.mv_mem.get());
    uint32_t* const mp = static_cast<uint32_t*>(v.mp_mem.get());
    minimizers_to_soa(right, v, mv, mp);
    for (int i = 0; i < n; ++i) {
        v.roff[size_t(i)] = rtot;
        ProcSeq* r = rep_of(right, i);
        if (!r) continue;
        if (!r->HpcSeq) die("Entry without HpcSeq in the right batch");
        v.state[size_t(i)] = 0;
        v.nmem[size_t(i)] = int32_t(right.Cls[size_t(i)]->size()) - 1;
        v.raw_len[size_t(i)] = uint32_t(r->RawSeq->seq.size());
        v.hpc_len[size_t(i)] = uint32_t(r->HpcSeq->seq.size());
        v.score[size_t(i)] = r->RawSeq->score;
        v.raw_err[size_t(i)] = r->RawSeq->errorRate;
        v.hpc_err[size_t(i)] = r->HpcSeq->errorRate;
        if (need_seq) rtot += int64_t(r->RawSeq->seq.size());
    }
    // the raw sequences side by side (alignment modes, consensus): one huge-page buffer, filled by a few threads
    v.rseq_mem = huge_alloc(size_t(rtot) + 1);
    char* const rseq = static_cast<char*>(v.rseq_mem.get());
    if (need_seq && rtot > 0) {
        const unsigned nt = host_threads(8);
        run_threads(nt, [&](unsigned t0) {
            for (int i = int(t0); i < n; i += int(nt))
                if (ProcSeq* r = rep_of(right, i)) memcpy(rseq + v.roff[size_t(i)], r->RawSeq->seq.data(), r->RawSeq->seq.size());
        });
    }
    v.roff[size_t(n)] = rtot;
    ioc_batch_view& rv = v.view;
    rv.n = n;
    rv.off_fwd = v.of.data();
    rv.off_rev = v.orv.data();
    rv.min_val = mv;
    rv.min_pos = mp;
    rv.total = tot;
    rv.raw_len = v.raw_len.data();
    rv.hpc_len = v.hpc_len.data();
    rv.score = v.score.data();
    rv.raw_err = v.raw_err.data();
    rv.hpc_err = v.hpc_err.data();
    rv.state = v.state.data();
    rv.min_qual = a.MinQual;
    rv.raw_seq = need_seq ? rseq : nullptr;
    rv.raw_off = need_seq ? v.roff.data() : nullptr;
    rv.n_members = v.nmem.data();
    rv.depth = right.Depth;
    rv.min_cls_size = a.MinClsSize;
}

// ---- left batch -> ioc_left_view ----
void flatten_left(const Batch& left, bool need_seq, LeftView& v)
{
    const int L = int(left.Cls.size());
    v.hpc_err.assign(static_cast<size_t>(L) + 1, 0.0), v.raw_err.assign(static_cast<size_t>(L) + 1, 0.0);
    v.off.assign(static_cast<size_t>(L) + 1, 0);
    for (int i = 0; i < L; ++i) {
        auto& cl = left.Cls[size_t(i)];
        if (!cl || cl->empty() || !cl->at(0) || !cl->at(0)->HpcSeq || !cl->at(0)->RawSeq) die("Left cluster without representative");
        v.hpc_err[size_t(i)] = cl->at(0)->HpcSeq->errorRate;
        v.raw_err[size_t(i)] = cl->at(0)->RawSeq->errorRate;
        v.off[size_t(i)] = int64_t(v.seq.size());
        if (need_seq) v.seq.append(cl->at(0)->RawSeq->seq.data(), cl->at(0)->RawSeq->seq.size());
    }
    v.off[size_t(L)] = int64_t(v.seq.size());
    v.k_offs.push_back(0);
    for (auto& kv : left.Db) {
        if (kv.second.empty()) continue;
        v.keys.push_back(kv.first);
        kv.second.append_to(v.post);
        v.k_offs.push_back(int64_t(v.post.size()));
    }
    ioc_left_view& lv = v.view;
    lv.n_clusters = L;
    lv.cls_hpc_err = v.hpc_err.data();
    lv.n_keys = int64_t(v.keys.size());
    lv.keys = v.keys.data();
    lv.offs = v.k_offs.data();
    lv.postings = v.post.data();
    lv.rep_seq = need_seq ? v.seq.data() : nullptr;
    lv.rep_off = need_seq ? v.off.data() : nullptr;
    lv.cls_raw_err = v.raw_err.data();
}

// the five graph operations go to the engine; rep_changed is ours: it records into the session of the job that is running
ConsensusSession* g_session = nullptr;
void record_rep_changed(void*, int32_t cls, const ioc_rep_record* rec)
{
    RepEvent& e = g_session->rep_events[cls];
    e.entry = rec->entry;
    e.raw.assign(rec->raw_seq, size_t(rec->raw_len));
    e.hpc.assign(rec->hpc_seq, size_t(rec->hpc_len));
    e.qual = rec->raw_qual;
    e.raw_err = rec->raw_err;
    e.raw_score = rec->raw_score;
    e.hpc_err = rec->hpc_err;
    e.mins.resize(size_t(rec->n_fwd));
    for (int32_t t = 0; t < rec->n_fwd; ++t) e.mins[size_t(t)] = Minimizer{rec->fwd_min[t], rec->fwd_pos[t], uint32_t(t)};
    e.rev.resize(size_t(rec->n_rev));
    for (int32_t t = 0; t < rec->n_rev; ++t) e.rev[size_t(t)] = Minimizer{rec->rev_min[t], rec->rev_pos[t], uint32_t(t)};
}

// the engine, the stored graphs of both sides, a seed for every left cluster without one, and the operations the driver calls
void open_consensus_session(ClusterJob& job)
{
    ConsensusSession& s = job.cons;
    ioc_ctx* const c = job.c;
    const Batch &left = job.left, &right = job.right;
    const int spoa_algo = job.opt.spoa_algo;
    // -A as src/main.cpp:292-318 reads it: 0 local, 1 global, 2 semi-global, anything else local (its line names no algorithm then)
    const int poa_type = (spoa_algo == IOC_POA_GLOBAL || spoa_algo == IOC_POA_SEMI_GLOBAL) ? spoa_algo : IOC_POA_LOCAL;
    if (VERBOSE)
        cerr << "Generating consensus using spoa algorithm: "
             << (spoa_algo == 0 ? "local" : spoa_algo == 1 ? "global" : spoa_algo == 2 ? "semi-global" : "") << endl;
    check(c, ioc_poa_create_mode(c, poa_type, 4, -8, -8, -4, -20, -1, &s.poa), "consensus engine");  // src/main.cpp:285-290
    auto load_side = [&](int side, const decltype(left.ConsGs)& gs, size_t limit, const char* what) {
        std::vector<int32_t> ids;
        std::vector<const uint8_t*> ptr;
        std::vector<int64_t> len;
        for (size_t i = 0; i < gs.size() && i < limit; ++i)
            if (!gs[i].empty()) {
                ids.push_back(int32_t(i));
                ptr.push_back(gs[i].data());
                len.push_back(int64_t(gs[i].size()));
            }
        check(c, ioc_poa_graph_load_many(s.poa, side, int32_t(ids.size()), ids.data(), ptr.data(), len.data()), what);
    };
    load_side(0, left.ConsGs, size_t(job.L), "left consensus graph");
    load_side(1, right.ConsGs, size_t(job.n), "right consensus graph");
    // left clusters without a stored graph (batches clustered without consensus): seeded with the representative
    for (int i = 0; i < job.L; ++i)
        if (size_t(i) >= left.ConsGs.size() || left.ConsGs[size_t(i)].empty()) {
            ioc_consensus_ops seed{};
            ioc_poa_bind(s.poa, &seed);
            const Bytes& rs0 = left.Cls[size_t(i)]->at(0)->RawSeq->seq;
            seed.create(seed.user, 0, i, rs0.data(), int(rs0.size()));
        }
    ioc_poa_bind(s.poa, &s.ops);
    g_session = &s;
    s.ops.user = s.poa;
    s.ops.rep_changed = record_rep_changed;
}

// the merge call, or the consensus call with its session
void run_core(ClusterJob& job)
{
    ioc_ctx* const c = job.c;
    const CmdArgs& a = job.left.SortArgs;
    const int mode = job.opt.mode;
    ioc_params p{a.KmerSize, a.WindowSize, a.MinShared, mode, a.MinFraction, a.MappedThreshold, a.MinProbNoHits, a.AlignedThreshold};
    const ioc_left_view* const lv = job.L > 0 ? &job.lv.view : nullptr;
    if (job.cons_on) {
        if (mode == None) die("Invalid clustering mode: 3");
        open_consensus_session(job);
        std::vector<int32_t> lsizes(static_cast<size_t>(job.L) + 1, 2);
        for (int i = 0; i < job.L; ++i) lsizes[size_t(i)] = int32_t(job.left.Cls[size_t(i)]->size());
        ioc_consensus_args ca{a.ConsMinSize, a.ConsMaxSize, a.ConsPeriod, job.left.Depth, lsizes.data()};
        check(c, ioc_cluster_consensus(c, &p, table_path().c_str(), lv, &job.rv.view, &ca, &job.cons.ops, job.out_cls.data(),
                                       job.out_strand.data(), &job.st),
              "clustering (consensus mode)");
    } else {
        check(c, ioc_cluster_merge(c, &p, table_path().c_str(), lv, &job.rv.view, job.out_cls.data(), job.out_strand.data(), &job.st),
              "clustering");
    }
}

// representative copies of the fresh reads that open clusters (cluster.cpp:181-199): the large fields are immutable views
// (cer.hpp), so a copy shares them — only the names are new
std::vector<std::shared_ptr<ProcSeq>> copy_fresh_representatives(const ClusterJob& job)
{
    const Batch &left = job.left, &right = job.right;
    const int n = job.n;
    std::vector<std::shared_ptr<ProcSeq>> rep_copy(static_cast<size_t>(n));
    std::vector<int> fresh;
    int next_id = int(left.Cls.size());
    std::vector<int> new_id(static_cast<size_t>(n), -1);
    for (int i = 0; i < n; ++i)
        if (job.out_cls[size_t(i)] >= 0 && job.out_cls[size_t(i)] == next_id) {
            new_id[size_t(i)] = next_id++;
            if (right.Cls[size_t(i)] && right.Cls[size_t(i)]->size() == 1 && rep_of(right, i)) fresh.push_back(i);
        }
    for (const int i : fresh) {
        ProcSeq* r = rep_of(right, i);
        auto rep = std::make_shared<ProcSeq>();
        rep->RawSeq.reset(new Seq(*r->RawSeq));
        rep->HpcSeq.reset(new Seq(*r->HpcSeq));
        rep->Mins = r->Mins;
        rep->RevMins = r->RevMins;
        rep->MatchStrand = r->MatchStrand;
        rep->Id = r->Id;
        const string nm = "rep_" + std::to_string(left.BatchNr) + "_" + std::to_string(new_id[size_t(i)]);
        rep->RawSeq->name = nm;
        rep->HpcSeq->name = nm;
        rep_copy[size_t(i)] = rep;
    }
    return rep_copy;
}

// ---- bookkeeping of the loop, cluster.cpp:115-310: the representative copies and the member moves ----
void apply_decisions(ClusterJob& job)
{
    Batch &left = job.left, &right = job.right;
    const CmdArgs& a = left.SortArgs;
    const std::vector<std::shared_ptr<ProcSeq>> rep_copy = copy_fresh_representatives(job);
    for (int i = 0; i < job.n; ++i) {
        auto& entry = right.Cls[size_t(i)];
        ProcSeq* r = rep_of(right, i);
        if (job.out_cls[size_t(i)] < 0) {
            if (r && r->RawSeq->score >= 0) {
                // gates that mark the read as unusable (cluster.cpp:148-160)
                if (r->RawSeq->seq.size() < size_t(2 * a.KmerSize) || r->HpcSeq->seq.size() < size_t(2 * a.KmerSize) ||
                    (-10 * log10(r->RawSeq->errorRate)) <= a.MinQual)
                    r->RawSeq->score = -1.0;
            }
            continue;
        }
        const int best = job.out_cls[size_t(i)];
        if (best == int(left.Cls.size())) {  // opens a new cluster (cluster.cpp:177-222)
            if (entry->size() == 1) {
                if (!rep_copy[size_t(i)]) die("Inconsistent cluster id from the device path");
                entry->insert(entry->begin(), rep_copy[size_t(i)]);
            }
            left.Cls.push_back(entry);
            left.NrCls++;
        } else {  // joins (cluster.cpp:223-261)
            if (best > int(left.Cls.size())) die("Inconsistent cluster id from the device path");
            for (auto& s : *entry) {
                if (!s) die("Null pointer in read array");
                if (job.out_strand[size_t(i)] == -1) {
                    if (s->MatchStrand == 1) s->MatchStrand = -1;
                    else if (s->MatchStrand == -1) s->MatchStrand = 1;
                    else die("Invalid match strand!");
                }
                s->Mins.clear();
                s->RevMins.clear();
                if (!job.opt.keep_seq) {
                    s->RawSeq.reset();
                    s->HpcSeq.reset();
                }
            }
            auto& dst = *left.Cls[size_t(best)];
            size_t from = entry->size() > 1 ? 1 : 0;
            for (size_t t = from; t < entry->size(); ++t) dst.push_back((*entry)[t]);
        }
    }
    left.Depth++;
    left.BatchEnd = right.BatchEnd;
    left.BatchBases += right.BatchBases;
}

// MinDB after AddMinimizers of every new representative
void import_index(ClusterJob& job)
{
    ioc_ctx* const c = job.c;
    Batch& left = job.left;
    int64_t nk = 0, np = 0;
    check(c, ioc_index_export(c, &nk, &np, nullptr, nullptr, nullptr), "index export");
    std::vector<uint32_t> ek(static_cast<size_t>(nk) + 1);
    auto ep = std::make_shared<std::vector<uint32_t>>(static_cast<size_t>(np) + 1);  // one flat array; the lists are views of it
    std::vector<int64_t> eo(static_cast<size_t>(nk) + 2);
    check(c, ioc_index_export(c, &nk, &np, ek.data(), eo.data(), ep->data()), "index export");
    left.Db.clear();
    left.Db.reserve(size_t(nk));
    for (int64_t i = 0; i < nk; ++i)
        left.Db.emplace_back(ek[size_t(i)], Span<uint32_t>(ep->data() + eo[size_t(i)], size_t(eo[size_t(i) + 1] - eo[size_t(i)]), ep));
}

// the -v summary, and the fields of the output batch that do not depend on the consensus
void report_and_label(ClusterJob& job)
{
    Batch& left = job.left;
    if (VERBOSE) {
        cerr << "Finished clustering!" << endl;
        cerr << "Alignment invocation count: " << job.st.n_aln_invoked << " (" << (job.n ? double(job.st.n_aln_invoked) / job.n * 100 : 0.0) << "%)" << endl;
        cerr << "Consensus invocation count: 0 (0%)" << endl;
        unsigned cnt = 0;
        for (auto& cl : left.Cls) cnt += cl->size() > 1;
        cerr << "Number of clusters larger than 1: " << cnt << endl;
        cerr << "Output batch statistics:" << endl;
        print_batch_info(left);
    }
    left.LeftLeaf = job.opt.left_path;
    left.RightLeaf = job.opt.right_path;
    if (job.opt.min_purge) {
        cerr << "Purging minimizer database in output batch!" << endl;
        left.Db.clear();
    }
    left.NrConsGs = left.Cls.size();
    left.ConsGs.clear();
}

// UpdateClusterConsensus' effect on the representatives (consensus.cpp:93-124), last event per cluster; then every cluster's graph
void apply_rep_events_and_save_graphs(ClusterJob& job)
{
    Batch& left = job.left;
    for (auto& kv : job.cons.rep_events) {
        if (kv.first < 0 || size_t(kv.first) >= left.Cls.size()) die("Inconsistent cluster id from the consensus path");
        auto& rep = left.Cls[size_t(kv.first)]->at(0);
        const RepEvent& e = kv.second;
        const string nm = "cons_" + std::to_string(left.BatchNr) + "_" + std::to_string(e.entry);
        rep->RawSeq.reset(new Seq);
        rep->RawSeq->name = nm;
        rep->RawSeq->seq = e.raw;
        rep->RawSeq->qual = string(e.raw.size(), e.qual);
        rep->RawSeq->score = e.raw_score;
        rep->RawSeq->errorRate = e.raw_err;
        rep->HpcSeq.reset(new Seq);
        rep->HpcSeq->name = nm;
        rep->HpcSeq->seq = e.hpc;
        rep->HpcSeq->qual = string(e.hpc.size(), e.qual);
        rep->HpcSeq->score = e.hpc_err * double(e.hpc.size());
        rep->HpcSeq->errorRate = e.hpc_err;
        rep->Mins = e.mins;
        rep->RevMins = e.rev;
    }
    left.ConsGs.resize(left.Cls.size());
    for (size_t i = 0; i < left.Cls.size(); ++i) {
        const int64_t sz = ioc_poa_graph_save(job.cons.poa, 0, int(i), nullptr, 0);
        if (sz <= 0) continue;
        left.ConsGs[i].resize(size_t(sz));
        if (ioc_poa_graph_save(job.cons.poa, 0, int(i), left.ConsGs[i].data(), sz) != sz) die("Failed to serialize a consensus graph");
    }
    if (VERBOSE) cerr << "Consensus invocation count: " << job.st.n_cons_invoked << endl;
}

void save_and_report(ClusterJob& job)
{
    string err;
    job.unlink_old.wait();
    auto t_save = Clock::now();
    if (!save_batch(job.left, job.opt.out_path, err)) die(err);
    job.save_ms = ms_since(t_save);
    const double cli_ms = ms_since(job.t_begin);
    if (VERBOSE) cerr << "Output batch written to: " << job.opt.out_path << endl;
    if (getenv("ISONCLUST2_STATS_JSON"))
        fprintf(stderr,
                "{\"entries\": %d, \"clusters\": %lld, \"core_ms\": %.3f, \"cli_ms\": %.3f, \"resolve_sweeps\": %d, "
                "\"load_ms\": %.3f, \"flatten_ms\": %.3f, \"ctx_ms\": %.3f, \"trim_ms\": %.3f, \"bookkeeping_ms\": %.3f, \"save_ms\": %.3f, "
                "\"t_begin_mono_ms\": %.3f, \"t_end_mono_ms\": %.3f}\n",
                job.n, (long long)job.st.n_clusters, job.core_ms, cli_ms, job.st.resolve_iters, job.load_ms, job.flatten_ms, job.ctx_ms, job.trim_ms,
                job.book_ms, job.save_ms,
                // (CLOCK_MONOTONIC, the clock of Python's time.monotonic(): a harness can tell the time before main and after _exit)
                std::chrono::duration<double, std::milli>(job.t_begin.time_since_epoch()).count(),
                std::chrono::duration<double, std::milli>(Clock::now().time_since_epoch()).count());
}

}  // namespace

int main_cluster(int argc, char** argv)
{
    ClusterJob job;
    job.opt = parse_cluster_options(argc, argv);
    job.t_begin = Clock::now();
    job.ctx_future = std::async(std::launch::async, start_context);
    load_inputs(job);
    flatten_right(job.right, job.need_seq, job.left.SortArgs, job.rv);
    flatten_left(job.left, job.need_seq, job.lv);
    job.flatten_ms = ms_since(job.t_begin) - job.load_ms;
    std::tie(job.c, job.ctx_ms) = job.ctx_future.get();
    job.out_cls.resize(static_cast<size_t>(job.n) + 1);
    job.out_strand.resize(static_cast<size_t>(job.n) + 1);

    job.t_core = Clock::now();
    run_core(job);
    job.core_ms = ms_since(job.t_core);
    // a one-shot process gives the aligner's arena back NOW, beside its own bookkeeping and writing: the driver wipes released
    // VRAM before anybody gets it again, and the next `cluster` process of a pipeline would wait for that in its own first
    // large allocation (0.27 ms or 400 ms for the same 8 GB hipMalloc: profiles/r05_cli_breakdown.txt)
    if (!g_served && (job.opt.mode == Sahlin || job.opt.mode == Furious)) (void)ioc_ctx_trim(job.c);
    job.trim_ms = ms_since(job.t_core) - job.core_ms;

    apply_decisions(job);
    import_index(job);
    report_and_label(job);
    if (job.cons_on) apply_rep_events_and_save_graphs(job);
    job.book_ms = ms_since(job.t_core) - job.core_ms - job.trim_ms;
    save_and_report(job);

    if (job.cons.poa && !g_served && getenv("IOC_TRACE")) ioc_poa_destroy(job.cons.poa);  // (prints the engine's counters)
    fflush(nullptr);
    if (g_served) return 0;  // (the resident process keeps its context; the batch records go with this frame)
    // the output is on disk: leave without unwinding a gigabyte of host structures and the HIP runtime
    std::cout.flush();
    cerr.flush();
    if (getenv("IOC_CLI_CLEAN_EXIT")) exit(0);  // (profilers write their results from exit handlers)
    _exit(0);
}
