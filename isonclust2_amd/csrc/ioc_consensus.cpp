// ioc_consensus.cpp — ClusterSortedReads with the consensus branch on (src/cluster.cpp:200-204, 263-309;
// src/consensus.cpp:34-137): SURVEY.md §8 f4.
//
// With ConsMaxSize > 0 a cluster's representative is REPLACED by a consensus after (almost) every join once its
// graph holds ConsMinSize sequences, which breaks the decision-independence the parallel resolve rests on
//  — but only at those events.  The driver therefore speculates: the device pipeline
// (index build, scoring, resolve, alignment fallback) runs over ALL remaining entries against the current
// left state; the host walks the decisions in the reference's order, doing its bookkeeping, until the first
// join that replaces a representative; decisions up to there are final, everything after is recomputed
// against the updated state.  The representative's new minimizers come from the GPU extractor (K1), the
// index edit is UpdateMinDB.
//
// spoa is absent from the reference tree: the partial-order graphs stay on the caller's side, behind the five
// operations the reference performs on them (ioc_consensus_ops), the way parasail can stay behind
// ioc_get_ties / ioc_set_aln_verdicts.  Nothing here links the oracle; without a device every call fails.
#include <algorithm>
#include <iterator>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <memory>
#include <vector>

#include "ioc_internal.h"

namespace {

// a graph operation of the caller failed: keep what it left in the context's error text (the shipped POA engine reports
// there), the caller of the ABI sees both
int hook_fail(ioc_ctx* c, const char* what)
{
    const std::string inner = c->err;
    return ioc_fail(c, IOC_ERR_INPUT, std::string("consensus hook: ") + what + " failed" + (inner.empty() ? "" : ": " + inner));
}

struct ClState {
    uint64_t seq_id = 0;             // identity of the representative's sequence (alignment results are kept by identity)
    double raw_err = 0, hpc_err = 0;
    int64_t size = 0;                // cls[c]->size(): representative copy + members
    std::vector<uint32_t> vals;      // sorted distinct forward minimizer values of the representative
    std::string raw;                 // representative's raw sequence (alignment fallback / ConsPurge)
    bool have_raw = false;
};

void sorted_unique(std::vector<uint32_t>& v)
{
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
}

// UpdateMinDB's removal (minimizer.cpp:143-147): the list sorted, made unique, without the cluster.  The lists are strictly
// ascending already unless a caller loaded something else: then the one entry is cut out in place.
void drop_cluster(std::vector<uint32_t>& lst, uint32_t cls)
{
    bool ascending = true;
    for (size_t x = 1; x < lst.size() && ascending; ++x) ascending = lst[x - 1] < lst[x];
    if (ascending) {
        auto it = std::lower_bound(lst.begin(), lst.end(), cls);
        if (it != lst.end() && *it == cls) lst.erase(it);
        return;
    }
    sorted_unique(lst);
    lst.erase(std::remove(lst.begin(), lst.end(), cls), lst.end());
}

// Values of the clusters whose representative changed during the current pass (old and new minimizer sets):
// a later entry of the pass keeps the decision the device made iff it shares fewer than
// int(MinShared * MinFraction) values with each of them — then none of them was, or becomes, a candidate that
// GetBestCluster looks at (cluster.cpp:324-406 walks candidates down to int(top * MinFraction), top >= MinShared).
struct DirtyIndex {
    static constexpr uint32_t CAP = 1u << 20, MASK = CAP - 1, EMPTY = 0xFFFFu;
    static constexpr int MAX_SLOTS = 256;  // clusters whose representative changes in one pass (deferred consensus batches that many events)
    std::vector<uint32_t> key = std::vector<uint32_t>(CAP, 0);
    std::vector<uint16_t> val = std::vector<uint16_t>(CAP, uint16_t(EMPTY));
    std::vector<uint32_t> touched;
    int nslots = 0;
    static uint32_t hash(uint32_t v) { return (v * 2654435761u) >> 12; }
    void reset()
    {
        for (uint32_t h : touched) val[h] = uint16_t(EMPTY);
        touched.clear();
        nslots = 0;
    }
    bool full() const { return nslots >= MAX_SLOTS || touched.size() > CAP / 4; }
    void add_cluster(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b)  // sorted, unique
    {
        std::vector<uint32_t> u;
        std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(u));
        for (uint32_t v : u) {
            uint32_t h = hash(v) & MASK;
            while (val[h] != EMPTY) h = (h + 1) & MASK;
            key[h] = v;
            val[h] = uint16_t(nslots);
            touched.push_back(h);
        }
        ++nslots;
    }
    // does the entry with these minimizer values (both strands' lists) reach `thr` shared values with any of them?
    bool touches(const uint32_t* v1, int64_t n1, const uint32_t* v2, int64_t n2, int thr) const
    {
        if (nslots == 0) return false;
        int cnt[MAX_SLOTS] = {0};
        for (int pass = 0; pass < 2; ++pass) {
            const uint32_t* v = pass ? v2 : v1;
            const int64_t nv = pass ? n2 : n1;
            for (int64_t x = 0; x < nv; ++x) {
                uint32_t h = hash(v[x]) & MASK;
                while (val[h] != EMPTY) {
                    if (key[h] == v[x] && ++cnt[val[h]] >= thr) return true;
                    h = (h + 1) & MASK;
                }
            }
        }
        return false;
    }
};

typedef std::vector<std::pair<int32_t, int8_t>> DepSet;

// The left state's MinDB on the host.  Hashed: UpdateMinDB looks up hundreds of keys per event, among half a million; where
// the reference's std::map order matters — the flat view, the export — the keys are sorted.
struct HostMinDB {
    std::unordered_map<uint32_t, std::vector<uint32_t>> db;
    // The MinDB as flat arrays.  Walking the map (half a million keys, a heap vector behind each) cost 10 ms per pass; a
    // pass touches a few thousand keys, so the arrays of the previous pass are patched instead: untouched stretches are
    // copied, the keys written since (dirty_keys: AddMinimizers, UpdateMinDB; a rollback only touches keys of its own pass)
    // are looked up in the map.
    std::vector<uint32_t> keys, post, keys2, post2, dirty_keys;
    std::vector<int64_t> offs, offs2;
    bool have_view = false;

    // the map and every cluster's value list; false: a posting names a cluster the left view does not have
    bool load(const ioc_left_view* left, std::vector<ClState>& cl)
    {
        if (!left) return true;
        if (left->n_keys > 0) db.reserve(size_t(left->n_keys) * 2);
        for (int64_t i = 0; i < left->n_keys; ++i) {
            auto& v = db[left->keys[i]];
            v.assign(left->postings + left->offs[i], left->postings + left->offs[i + 1]);
            for (uint32_t t : v) {
                if (t >= cl.size()) return false;
                cl[t].vals.push_back(left->keys[i]);  // keys ascending -> vals come out sorted
            }
        }
        return true;
    }
    // AddMinimizers (minimizer.cpp:31-42): the new id is larger than every id in the lists.  key_was_new: per value, whether
    // this opened the key
    void add_cluster(const std::vector<uint32_t>& vals, uint32_t id, std::vector<uint8_t>* key_was_new)
    {
        if (key_was_new) {
            key_was_new->reserve(vals.size());
            for (uint32_t v : vals) key_was_new->push_back(db.find(v) == db.end() ? 1 : 0);
        }
        for (uint32_t v : vals) db[v].push_back(id);
        dirty_keys.insert(dirty_keys.end(), vals.begin(), vals.end());
    }
    // UpdateMinDB (minimizer.cpp:124-160); upd_keys collects the keys it went through (db[v] opens a key, even an empty one)
    void update(uint32_t id, const std::vector<uint32_t>& old_vals, const std::vector<uint32_t>& new_vals, std::vector<uint32_t>* upd_keys)
    {
        std::vector<uint32_t> to_del, to_ins;
        std::set_difference(old_vals.begin(), old_vals.end(), new_vals.begin(), new_vals.end(), std::back_inserter(to_del));
        std::set_difference(new_vals.begin(), new_vals.end(), old_vals.begin(), old_vals.end(), std::back_inserter(to_ins));
        for (uint32_t v : to_del) drop_cluster(db[v], id);
        for (uint32_t v : to_ins) {
            auto& lst = db[v];
            lst.push_back(id);
            std::sort(lst.begin(), lst.end());
        }
        for (const auto* ks : {&to_del, &to_ins}) {
            dirty_keys.insert(dirty_keys.end(), ks->begin(), ks->end());
            if (upd_keys) upd_keys->insert(upd_keys->end(), ks->begin(), ks->end());
        }
    }
    // takes add_cluster back, newest value first (upd_keys sorted); false: a list no longer ends with the cluster
    bool undo_add(uint32_t id, const std::vector<uint32_t>& vals, const std::vector<uint8_t>& key_was_new, const std::vector<uint32_t>& upd_keys)
    {
        for (size_t y = vals.size(); y-- > 0;) {
            auto it = db.find(vals[y]);
            if (it == db.end() || it->second.empty() || it->second.back() != id) return false;
            it->second.pop_back();
            // the key goes with the cluster that opened it — unless an event that stands went through it
            // since (in the reference's order UpdateMinDB's db[v] would have opened it, minimizer.cpp:143-152)
            if (key_was_new[y] && it->second.empty() && !std::binary_search(upd_keys.begin(), upd_keys.end(), vals[y])) db.erase(it);
        }
        return true;
    }
    // the map as flat arrays, keys ascending (lists emptied by UpdateMinDB stay in the MinDB but match nothing: a view leaves them out)
    void flat(bool with_empty, std::vector<uint32_t>& K, std::vector<int64_t>& O, std::vector<uint32_t>& P) const
    {
        K.clear();
        O.clear();
        P.clear();
        K.reserve(db.size());
        for (auto& kv : db)
            if (with_empty || !kv.second.empty()) K.push_back(kv.first);
        std::sort(K.begin(), K.end());
        for (uint32_t k2 : K) {
            const auto& lst = db.find(k2)->second;
            O.push_back(int64_t(P.size()));
            P.insert(P.end(), lst.begin(), lst.end());
        }
        O.push_back(int64_t(P.size()));
    }
    void patch()  // keys2 / offs2 / post2 from the previous arrays and dirty_keys, then swapped in
    {
        std::sort(dirty_keys.begin(), dirty_keys.end());
        dirty_keys.erase(std::unique(dirty_keys.begin(), dirty_keys.end()), dirty_keys.end());
        keys2.clear();
        offs2.clear();
        post2.clear();
        keys2.reserve(keys.size() + dirty_keys.size());
        offs2.reserve(keys.size() + dirty_keys.size() + 1);
        post2.reserve(post.size() + post.size() / 16 + 4096);
        const size_t nk = keys.size();
        size_t a = 0;
        auto copy_range = [&](size_t from, size_t to) {  // entries [from, to) of the previous arrays, as they are
            if (from >= to) return;
            const int64_t delta = int64_t(post2.size()) - offs[from];
            keys2.insert(keys2.end(), keys.begin() + int64_t(from), keys.begin() + int64_t(to));
            const size_t o = offs2.size();
            offs2.resize(o + (to - from));
            for (size_t x = from; x < to; ++x) offs2[o + (x - from)] = offs[x] + delta;
            post2.insert(post2.end(), post.begin() + offs[from], post.begin() + offs[to]);
        };
        for (uint32_t dk : dirty_keys) {
            const size_t b = size_t(std::lower_bound(keys.begin() + int64_t(a), keys.end(), dk) - keys.begin());
            copy_range(a, b);
            a = b;
            if (a < nk && keys[a] == dk) ++a;
            auto it = db.find(dk);
            if (it != db.end() && !it->second.empty()) {
                keys2.push_back(dk);
                offs2.push_back(int64_t(post2.size()));
                post2.insert(post2.end(), it->second.begin(), it->second.end());
            }
        }
        copy_range(a, nk);
        offs2.push_back(int64_t(post2.size()));
        keys.swap(keys2);
        offs.swap(offs2);
        post.swap(post2);
    }
    // keys / offs / post as the map stands; check (IOC_CONS_VIEW_CHECK=1): also rebuilt from the map, false if the two differ
    bool view(bool check)
    {
        if (!have_view)
            flat(false, keys, offs, post);
        else if (!dirty_keys.empty())
            patch();
        have_view = true;
        dirty_keys.clear();
        if (!check) return true;
        flat(false, keys2, offs2, post2);
        return keys2 == keys && offs2 == offs && post2 == post;
    }
    void export_to(ioc_ctx* c) const  // the final MinDB is what ioc_index_export returns
    {
        flat(true, c->exp_keys, c->exp_offs, c->exp_post);
        c->exp_valid = true;
    }
};

// The reference's hit order (GetMinimizerHits + SortMinimizerHits, minimizer.cpp:44-121) of entry i under the MinDB as it
// stands, clusters below `ncl` only: the same unordered_map (hash, initial bucket count, insertion sequence: forward
// minimizers in order, each posting list in order, then the reverse ones), the same std::sort.  The first candidate of `dep`
// in that order is what an order-dependent decision comes to (§3 of DESIGN.md): the candidates themselves — clusters
// whose representatives did not change — keep their Sizes and verdicts, only their order can move.
bool host_order_pick(const HostMinDB& mdb, const ioc_batch_view* rb, int i, int32_t ncl, const DepSet& dep, int32_t& w_cls, int8_t& w_strand)
{
    typedef std::pair<int, int> SCl;
    struct SClHash {
        std::size_t operator()(const SCl& u) const { return size_t(int(u.first * u.second)); }
    };
    struct SHit {
        unsigned Size, Cls;
        int Strand;
    };
    const int64_t nf = rb->off_fwd[i + 1] - rb->off_fwd[i], nr = rb->off_rev[i + 1] - rb->off_rev[i];
    std::unordered_map<SCl, unsigned, SClHash> res(size_t(20) * size_t(nf + nr), SClHash());
    for (int pass = 0; pass < 2; ++pass) {
        const uint32_t* v = rb->min_val + (pass ? rb->off_rev[i] : rb->off_fwd[i]);
        const int64_t nv = pass ? nr : nf;
        for (int64_t x = 0; x < nv; ++x) {
            auto it = mdb.db.find(v[x]);
            if (it == mdb.db.end()) continue;
            for (uint32_t cid2 : it->second)
                if (int32_t(cid2) < ncl) res[std::make_pair(int(cid2), pass ? -1 : 1)]++;
        }
    }
    std::vector<std::unique_ptr<SHit>> order;
    order.reserve(res.size());
    for (auto& kv : res) order.push_back(std::unique_ptr<SHit>(new SHit{kv.second, unsigned(kv.first.first), kv.first.second}));
    std::sort(order.begin(), order.end(), [](const std::unique_ptr<SHit>& a, const std::unique_ptr<SHit>& b) { return a->Size > b->Size; });
    for (auto& o : order)
        for (auto& d : dep)
            if (int32_t(o->Cls) == d.first && o->Strand == int(d.second)) {
                w_cls = d.first;
                w_strand = d.second;
                return true;
            }
    return false;
}

// One device pass over the window [pos, pos + m): what ioc_cluster_merge decided per window entry, and the buffers its
// views were built in (kept between passes for their capacity).
struct Pass {
    int pos = 0, m = 0;
    std::vector<int32_t> cls, cut;  // decision; the Size the entry's mapping walk stops at (ioc_get_cuts)
    std::vector<int8_t> strand;
    std::vector<uint8_t> flg, dep;
    std::vector<DepSet> depset;   // per window entry with dep: the candidates its hit order chooses among
    std::vector<int32_t> ncl_at;  // clusters that existed when the walk reached the window entry
    std::vector<int64_t> of, orv, roff, loff;
    std::vector<uint32_t> wval, wpos;
    std::vector<double> herr, rerr;
    std::string lseq;
    std::vector<int32_t> tgt;  // (tgt, str: never read — ioc_get_decisions fills all three of its buffers)
    std::vector<int8_t> str;
    bool order_dep(int x) const { return dep[size_t(x)] && !depset[size_t(x)].empty(); }
};

struct PendingEvent {  // a join that replaces the representative of cluster dc
    int x, i;
    int32_t dc;
    double hpc_err, raw_err;
    std::string cons;  // the consensus, once taken or collected
};
struct Undo {
    int kind, x;  // 0 gated, 1 new cluster, 2 join
    int32_t dc;
    int64_t dsize;
    std::vector<uint8_t> key_was_new;  // new cluster: per value, whether AddMinimizers opened the key
};
// A stretch of a pass walked on the same device decisions.  Deferred consensus (ioc_consensus_spec_ops; IOC_CONS_SPECULATE=0
// switches it off): the walk does not wait for a consensus — it records the event, queues the request and goes on as long
// as the entries it meets cannot see the OLD representative of a cluster with a pending event.  At the end of the segment
// all requested consensus sequences come back from ONE flush of the graph store (their additions aligned together), the new
// representatives are re-minimized by ONE extractor launch, and the entries walked after each event are checked again, in
// order, against old AND new minimizer sets — the reference's result is a function of those sets only.  An entry that
// could see a new representative after all ends the pass there: host state is undone from the journal, the graph
// store rolls back the operations tagged with later entries.
struct Segment {
    std::vector<PendingEvent> evs;
    std::vector<Undo> journal;       // what the walk did since the first event (before it nothing is ever undone)
    std::vector<uint32_t> upd_keys;  // keys UpdateMinDB went through in the verification
};
struct NewReps {  // consensus sequences through the extractor: per sequence e the lists [xf[e], xf[e + 1]) and [xr[e], xr[e + 1]) of mv / mp
    std::vector<int64_t> xoff, xf, xr;
    std::vector<uint32_t> hlen, mv, mp;
    std::vector<char> qraw, hs;
};
// How a walk ended, at window entry x: the whole window stands (x = m), the segment stops
// in front of x, it stops there and the walk resumes from x afterwards, or (consensus taken at once) the next pass starts at x.
enum class Walk { Whole, Stop, Resume, Restart };
struct WalkEnd {
    int rc;  // IOC_OK, or the call fails with it
    Walk how;
    int x;
};
enum Phase { PH_LEFT_VIEW, PH_DEVICE, PH_HOOKS, PH_NEW_REP, PH_FLUSH, PH_COLLECT, PH_VERIFY, PH_ROLLBACK, PH_COUNT };  // IOC_TRACE's clock

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// What lives across the passes of one ioc_cluster_consensus call.
struct Driver {
    ioc_ctx* c;
    const ioc_params* p;
    const char* table_path;
    const ioc_batch_view* rb;
    const ioc_consensus_args* ca;
    const ioc_consensus_ops* ops;
    int32_t* out_cls;
    int8_t* out_strand;
    const int n;
    const bool aln_mode;
    // ---- left state on the host: the MinDB, one ClState per cluster ----
    HostMinDB mdb;
    std::vector<ClState> cl;
    uint64_t next_seq_id;  // sequence identities: right entry i -> i; left representatives and consensus sequences -> n, n + 1, ...
    ioc_cluster_stats total{};
    // ALN_INVOKED (cluster.cpp:21, 559): an entry counts iff it reached the alignment fallback in the pass whose decision
    // stands for it — the flag of an entry is overwritten whenever a later pass walks it again
    std::vector<uint8_t> aln_flag;
    // A pass decides a WINDOW of entries, not all that remain: a decision depends on earlier entries only, so a
    // prefix of the batch gives the same decisions, and everything behind the next consensus event would be thrown
    // away anyway.  The window follows the distance between events (fast mode: thousands of entries, sahlin mode
    // with small clusters: a handful).
    int window;
    const bool fixed_window = getenv("IOC_CONS_WINDOW") != nullptr;
    const int pass_cap = ioc_pass_entries();
    DirtyIndex dirty;    // representatives changed (at once) or about to change (deferred) in this segment
    DirtyIndex dirty_b;  // (deferred) every representative replaced since the device pass
    // (the smallest Size a walk can reach: int(MinShared * MinFraction) in the mapping, but never above MinShared — with
    // MinFraction > 1 the mapping walks nothing and the alignment fallback still tries the candidates of Size top >= MinShared)
    const int dirty_thr;
    double ph[PH_COUNT] = {};
    int64_t n_spec_rollbacks = 0, n_spec_events = 0, n_spec_flushes = 0, rb_counter = 0;
    const ioc_consensus_spec_ops* spec;  // null: every consensus is taken at once
    const bool trace = getenv("IOC_TRACE") != nullptr, view_check = getenv("IOC_CONS_VIEW_CHECK") != nullptr;
    // IOC_CONS_FORCE_ROLLBACK=N (tests): every N-th entry looked at again is treated as if it could see a new
    // representative — a rollback only repeats work, the result must not change
    const int force_rb = getenv("IOC_CONS_FORCE_ROLLBACK") ? std::max(0, atoi(getenv("IOC_CONS_FORCE_ROLLBACK"))) : 0;
    std::vector<char> buf = std::vector<char>(size_t(1) << 22);  // a consensus as the graph store hands it over

    Driver(ioc_ctx* c_, const ioc_params* p_, const char* table, const ioc_batch_view* rb_, const ioc_consensus_args* ca_,
           const ioc_consensus_ops* ops_, int32_t* oc, int8_t* os)
        : c(c_), p(p_), table_path(table), rb(rb_), ca(ca_), ops(ops_), out_cls(oc), out_strand(os), n(rb_->n),
          aln_mode(p_->mode == IOC_MODE_SAHLIN || p_->mode == IOC_MODE_FURIOUS), next_seq_id(uint64_t(rb_->n)),
          aln_flag(size_t(rb_->n) + 1, 0), window(rb_->n),
          dirty_thr(std::max(1, std::min(p_->min_shared, int(double(p_->min_shared) * p_->min_fraction)))), spec(ops_->spec)
    {
        if (const char* e = getenv("IOC_CONS_WINDOW")) window = std::max(1, atoi(e));
        if (const char* e = getenv("IOC_CONS_SPECULATE"))
            if (atoi(e) == 0) spec = nullptr;
    }
    void next_window(bool restarted, int advanced)
    {
        if (fixed_window) return;
        // restarted: the next event is probably as far away as this one was
        window = restarted ? std::max(64, 4 * std::max(1, advanced)) : std::min(n, std::max(64, 2 * window));
    }

    int load(const ioc_left_view* left)
    {
        const int32_t L0 = left ? left->n_clusters : 0;
        cl.resize(size_t(L0));
        for (int32_t t = 0; t < L0; ++t) {
            cl[size_t(t)].seq_id = next_seq_id++;
            cl[size_t(t)].hpc_err = left->cls_hpc_err[t];
            cl[size_t(t)].raw_err = left->cls_raw_err ? left->cls_raw_err[t] : 0.0;
            cl[size_t(t)].size = ca->left_sizes ? ca->left_sizes[t] : 2;
            if (left->rep_seq && left->rep_off) {
                cl[size_t(t)].raw.assign(left->rep_seq + left->rep_off[t], size_t(left->rep_off[t + 1] - left->rep_off[t]));
                cl[size_t(t)].have_raw = true;
            }
        }
        return mdb.load(left, cl) ? IOC_OK : ioc_fail(c, IOC_ERR_ARG, "left posting >= n_clusters");
    }

    // The left view of the current state and the entries [pos, pos + m) as a batch view, through the device pipeline.
    int run_pass(Pass& ps, int pos)
    {
        const int m = std::min(std::min(n - pos, window), pass_cap);  // (no window beyond one device pass)
        ps.pos = pos;
        ps.m = m;
        double t0 = now_ms();
        const int32_t Lc = int32_t(cl.size());
        if (!mdb.view(view_check)) return ioc_fail(c, IOC_ERR_STATE, "consensus driver: the patched left view differs from a rebuilt one");
        ps.herr.resize(size_t(Lc));
        ps.rerr.resize(size_t(Lc));
        c->aln_lid.resize(size_t(Lc));
        for (int32_t t = 0; t < Lc; ++t) {
            ps.herr[size_t(t)] = cl[size_t(t)].hpc_err;
            ps.rerr[size_t(t)] = cl[size_t(t)].raw_err;
            c->aln_lid[size_t(t)] = cl[size_t(t)].seq_id;
        }
        c->aln_qid.resize(size_t(m));
        for (int i = 0; i < m; ++i) c->aln_qid[size_t(i)] = uint64_t(pos + i);
        ioc_left_view lv{};
        lv.n_clusters = Lc;
        lv.cls_hpc_err = ps.herr.data();
        lv.n_keys = int64_t(mdb.keys.size());
        lv.keys = mdb.keys.data();
        lv.offs = mdb.offs.data();
        lv.postings = mdb.post.data();
        if (aln_mode) {
            ps.lseq.clear();
            ps.loff.assign(size_t(Lc) + 1, 0);
            for (int32_t t = 0; t < Lc; ++t) {
                if (!cl[size_t(t)].have_raw) return ioc_fail(c, IOC_ERR_STATE, "a representative's sequence is missing");
                ps.lseq += cl[size_t(t)].raw;
                ps.loff[size_t(t) + 1] = int64_t(ps.lseq.size());
            }
            lv.rep_seq = ps.lseq.data();
            lv.rep_off = ps.loff.data();
            lv.cls_raw_err = ps.rerr.data();
        }
        // ---- the entries [pos, pos + m) as a batch view: their forward lists, then their reverse lists ----
        const int64_t fb = rb->off_fwd[pos], fe = rb->off_fwd[pos + m], vb = rb->off_rev[pos], ve = rb->off_rev[pos + m];
        const int64_t nf = fe - fb, nr = ve - vb;
        ps.wval.resize(size_t(nf + nr) + 1);
        ps.wpos.resize(size_t(nf + nr) + 1);
        std::copy(rb->min_val + fb, rb->min_val + fe, ps.wval.begin());
        std::copy(rb->min_val + vb, rb->min_val + ve, ps.wval.begin() + nf);
        std::copy(rb->min_pos + fb, rb->min_pos + fe, ps.wpos.begin());
        std::copy(rb->min_pos + vb, rb->min_pos + ve, ps.wpos.begin() + nf);
        ps.of.resize(size_t(m) + 1);
        ps.orv.resize(size_t(m) + 1);
        ps.roff.resize(size_t(m) + 1);
        for (int i = 0; i <= m; ++i) {
            ps.of[size_t(i)] = rb->off_fwd[pos + i] - fb;
            ps.orv[size_t(i)] = nf + (rb->off_rev[pos + i] - vb);
            ps.roff[size_t(i)] = rb->raw_off[pos + i] - rb->raw_off[pos];
        }
        ioc_batch_view sv = *rb;
        sv.n = m;
        sv.off_fwd = ps.of.data();
        sv.off_rev = ps.orv.data();
        sv.min_val = ps.wval.data();
        sv.min_pos = ps.wpos.data();
        sv.total = nf + nr;
        sv.raw_len = rb->raw_len + pos;
        sv.hpc_len = rb->hpc_len + pos;
        sv.score = rb->score + pos;
        sv.raw_err = rb->raw_err + pos;
        sv.hpc_err = rb->hpc_err + pos;
        sv.state = rb->state ? rb->state + pos : nullptr;
        sv.raw_seq = rb->raw_seq + rb->raw_off[pos];
        sv.raw_off = ps.roff.data();
        sv.n_members = rb->n_members ? rb->n_members + pos : nullptr;
        ps.cls.assign(size_t(m) + 1, -1);
        ps.strand.assign(size_t(m) + 1, 0);
        ioc_cluster_stats st{};
        ph[PH_LEFT_VIEW] += now_ms() - t0;
        t0 = now_ms();
        int r = ioc_cluster_merge(c, p, table_path, Lc > 0 ? &lv : nullptr, &sv, ps.cls.data(), ps.strand.data(), &st);
        if (r != IOC_OK) return r;
        ps.cut.assign(size_t(m) + 1, INT32_MAX);
        if (m > 0 && (r = ioc_get_cuts(c, ps.cut.data())) != IOC_OK) return r;
        ps.tgt.assign(size_t(m) + 1, 0);
        ps.str.assign(size_t(m) + 1, 0);
        ps.flg.assign(size_t(m) + 1, 0);
        if (m > 0 && (r = ioc_get_decisions(c, ps.tgt.data(), ps.str.data(), ps.flg.data())) != IOC_OK) return r;
        ps.dep.assign(size_t(m) + 1, 0);
        ps.depset.assign(size_t(m) + 1, DepSet());
        for (int x = 0; x < m && size_t(x) < c->last_order_dep.size(); ++x) {
            ps.dep[size_t(x)] = c->last_order_dep[size_t(x)];
            if (ps.dep[size_t(x)] && size_t(x) < c->last_dep_set.size()) ps.depset[size_t(x)] = c->last_dep_set[size_t(x)];
        }
        ps.ncl_at.assign(size_t(m) + 1, 0);
        ph[PH_DEVICE] += now_ms() - t0;
        total.resolve_iters += st.resolve_iters;
        total.n_tie_replays += st.n_tie_replays;
        total.aln_rounds += st.aln_rounds;
        total.n_aln_pairs += st.n_aln_pairs;
        total.n_cons_restarts++;
        if (trace) fprintf(stderr, "[ioc] consensus pass from entry %d (%d left clusters)\n", pos, Lc);
        return IOC_OK;
    }

    // Can window entry x see one of the changed representatives?  The device's decision for it stands only if it cannot — it
    // shares fewer values with each than the Size its mapping walk stops at (int(top * MinFraction), ioc_get_cuts; without a
    // walk: what would start one).  A decision that hangs on the reference's hit ORDER — a tie at the top Size, several candidates
    // that align — depends on which (cluster, strand) keys the hit map holds at all and on their Sizes, down to Size 1: the
    // iteration order of the unordered_map and the path of its std::sort change with them.  ONE value shared with a changed
    // representative's old or new set can add, remove or resize such a key.  Where the candidates the order chooses among are
    // known (depset), the order itself is computed again on the host (repick, verify_segment).
    bool can_see(const DirtyIndex& di, const Pass& ps, int x) const
    {
        const int i = ps.pos + x;
        const int thr = ps.cut[size_t(x)] == INT32_MAX ? dirty_thr : std::max(dirty_thr, int(ps.cut[size_t(x)]));
        return di.touches(rb->min_val + rb->off_fwd[i], rb->off_fwd[i + 1] - rb->off_fwd[i], rb->min_val + rb->off_rev[i],
                          rb->off_rev[i + 1] - rb->off_rev[i], (ps.dep[size_t(x)] && ps.depset[size_t(x)].empty()) ? 1 : thr);
    }

    // Takes the order-dependent decision of window entry x again: the order as it is now, the MinDB being exact.
    int repick(Pass& ps, int x)
    {
        int32_t wc = -1;
        int8_t ws = 0;
        if (!host_order_pick(mdb, rb, ps.pos + x, int32_t(cl.size()), ps.depset[size_t(x)], wc, ws))
            return ioc_fail(c, IOC_ERR_STATE, "consensus driver: none of an order-dependent decision's candidates is a hit any more");
        ps.cls[size_t(x)] = wc;
        ps.strand[size_t(x)] = ws;
        return IOC_OK;
    }

    // (verification) Does the order-dependent decision of window entry x come out as it was taken, among the clusters of that moment?
    bool same_pick(const Pass& ps, int x) const
    {
        if (!ps.order_dep(x) || ps.cls[size_t(x)] >= ps.ncl_at[size_t(x)]) return true;
        int32_t wc = -1;
        int8_t ws = 0;
        return host_order_pick(mdb, rb, ps.pos + x, ps.ncl_at[size_t(x)], ps.depset[size_t(x)], wc, ws) && wc == ps.cls[size_t(x)] && ws == ps.strand[size_t(x)];
    }

    // Walks the decisions from window entry x_begin in the reference's order until a representative changes (deferred: until
    // an entry could see a cluster with a pending event, or one replaced in an earlier segment of this device pass).
    WalkEnd walk_segment(Pass& ps, Segment& sg, int x_begin)
    {
        const auto fail = [](int rc) { return WalkEnd{rc, Walk::Stop, 0}; };
        dirty.reset();
        for (int x = x_begin; x < ps.m; ++x) {
            const int i = ps.pos + x;
            const int32_t& dc = ps.cls[size_t(x)];  // (repick may write it again)
            ps.ncl_at[size_t(x)] = int32_t(cl.size());
            aln_flag[size_t(i)] = dc >= 0 && (ps.flg[size_t(x)] & 2) ? 1 : 0;
            if (dc < 0) {  // (gated by its quality: no cluster has a say)
                out_cls[i] = -1;
                out_strand[i] = 0;
                total.n_gated++;
                if (spec && !sg.evs.empty()) sg.journal.push_back(Undo{0, x, -1, 0, {}});
                continue;
            }
            if (spec && dirty_b.nslots && (dirty_b.full() || can_see(dirty_b, ps, x))) return {IOC_OK, Walk::Stop, x};  // the device pass ends here
            // (deferred: it sees the OLD representative of a cluster with a pending event)
            if (dirty.nslots && can_see(dirty, ps, x)) return {IOC_OK, spec ? Walk::Stop : Walk::Restart, x};
            if (ps.order_dep(x) && dc < int32_t(cl.size())) {
                // requests pending: the segment ends in front of this entry, the walk goes on from it afterwards
                if (spec && !sg.evs.empty()) return {IOC_OK, Walk::Resume, x};
                if (spec ? dirty_b.nslots : dirty.nslots)
                    if (const int r = repick(ps, x)) return fail(r);
            }
            const char* rseq = rb->raw_seq + rb->raw_off[i];
            const int rlen = int(rb->raw_off[i + 1] - rb->raw_off[i]);
            const int64_t entry_size = rb->n_members ? int64_t(rb->n_members[i]) + 1 : 1;  // reads[i]->size()
            const bool undoable = spec && !sg.evs.empty();  // (before the first event of a segment nothing is ever undone: no snapshot needed)
            if (dc == int32_t(cl.size())) {
                // ---- opens a new cluster (cluster.cpp:177-222) ----
                ClState ns;
                ns.seq_id = uint64_t(i);  // the representative is this read
                ns.raw_err = rb->raw_err[i];
                ns.hpc_err = rb->hpc_err[i];
                ns.size = entry_size == 1 ? 2 : entry_size;  // a fresh read gets a representative copy in front
                ns.vals.assign(rb->min_val + rb->off_fwd[i], rb->min_val + rb->off_fwd[i + 1]);
                sorted_unique(ns.vals);
                ns.raw.assign(rseq, size_t(rlen));
                ns.have_raw = true;
                if (undoable) sg.journal.push_back(Undo{1, x, dc, 0, {}});
                mdb.add_cluster(ns.vals, uint32_t(dc), undoable ? &sg.journal.back().key_was_new : nullptr);
                if ((undoable ? spec->create_tagged(ops->user, 0, dc, rseq, rlen, i) : ops->create(ops->user, 0, dc, rseq, rlen)) < 0)
                    return fail(hook_fail(c, "create"));
                cl.push_back(std::move(ns));
                out_cls[i] = dc;
                out_strand[i] = 1;
                continue;
            }
            if (dc > int32_t(cl.size())) return fail(ioc_fail(c, IOC_ERR_STATE, "inconsistent cluster id from the device path"));
            // ---- joins cluster dc (cluster.cpp:223-309) ----
            ClState& b = cl[size_t(dc)];
            out_cls[i] = dc;
            out_strand[i] = ps.strand[size_t(x)];
            total.n_joined++;
            b.size += entry_size > 1 ? entry_size - 1 : 1;
            if (undoable) sg.journal.push_back(Undo{2, x, dc, entry_size > 1 ? entry_size - 1 : 1, {}});
            if (ca->cons_max_size <= 0) continue;
            if (ca->left_depth == -1 && ca->cons_period > 0 && b.size > ca->cons_period) continue;   // :267-271
            const int cons_min = ca->left_depth != -1 ? 2 : ca->cons_min_size;                           // :284-288
            // UpdateClusterConsensus, consensus.cpp:34-126
            const int left_size = ops->size(ops->user, 0, dc);
            if (left_size < 0) return fail(ioc_fail(c, IOC_ERR_INPUT, "consensus hook: the cluster has no graph"));
            const int rsz = ops->size(ops->user, 1, i);
            const bool have_right = rsz >= 0;
            const int right_size = have_right ? rsz : 1;
            const double hpc_err = (b.hpc_err * double(left_size) + rb->hpc_err[i] * double(right_size)) / double(left_size + right_size);
            const double raw_err = (b.raw_err * double(left_size) + rb->raw_err[i] * double(right_size)) / double(left_size + right_size);
            // (the reference reverse-complements a copy and throws it away, consensus.cpp:47-49: the read goes in as it is)
            double t0 = now_ms();
            if ((spec ? spec->add_tagged(ops->user, 0, dc, rseq, rlen, have_right ? unsigned(right_size) : 1u, i)
                      : ops->add(ops->user, 0, dc, rseq, rlen, have_right ? unsigned(right_size) : 1u)) < 0)
                return fail(hook_fail(c, "add"));
            ph[PH_HOOKS] += now_ms() - t0;
            if (ops->size(ops->user, 0, dc) < cons_min) continue;
            PendingEvent ev{x, i, dc, hpc_err, raw_err, std::string()};
            if (spec) {
                // ---- the consensus is requested, not awaited ----
                if (spec->consensus_deferred(ops->user, 0, dc, i) < 0) return fail(hook_fail(c, "deferred consensus"));
                sg.evs.push_back(std::move(ev));
                dirty.add_cluster(b.vals, std::vector<uint32_t>());  // what later entries must not see: the OLD set for now
                n_spec_events++;
                if (dirty.full()) return {IOC_OK, Walk::Stop, x + 1};
                continue;
            }
            t0 = now_ms();
            int r = take_consensus(ops->consensus(ops->user, 0, dc, buf.data(), int(buf.size())), ev.cons);
            if (r != IOC_OK) return fail(r);
            ph[PH_HOOKS] += now_ms() - t0;
            t0 = now_ms();
            const std::vector<PendingEvent> one(1, std::move(ev));
            NewReps nr;
            if ((r = new_representatives(one, nr)) != IOC_OK || (r = install_representative(one[0], nr, 0, dirty, nullptr)) != IOC_OK)
                return fail(r);
            ph[PH_NEW_REP] += now_ms() - t0;
            // every later entry that can see this cluster has to see the new representative: the walk goes on
            // until it meets one (can_see at the top), or restarts here when too many clusters have changed
            if (dirty.full()) return {IOC_OK, Walk::Restart, x + 1};
        }
        return {IOC_OK, Walk::Whole, ps.m};
    }

    // A consensus of clen characters in buf, as the graph store's consensus / collect returned it.
    int take_consensus(int clen, std::string& cons)
    {
        if (clen < 0) return hook_fail(c, "consensus");
        cons.assign(buf.data(), size_t(clen));
        if (!(cons.size() > size_t(2 * p->k) || cons.size() >= size_t(p->w)))
            return ioc_fail(c, IOC_ERR_INPUT, "consensus shorter than 2k and w (the reference re-minimizes an empty sequence here)");
        return IOC_OK;
    }

    // The new representatives: fixed quality character, HPC, minimizers (K1 on the GPU) — ONE extractor call for all of them.
    int new_representatives(const std::vector<PendingEvent>& evs, NewReps& nr)
    {
        const size_t ne = evs.size();
        nr.xoff.assign(ne + 1, 0);
        nr.qraw.resize(ne);
        std::string xseq, xqual;
        for (size_t e = 0; e < ne; ++e) {
            nr.qraw[e] = std::to_string(int(-10 * log10(evs[e].raw_err)) + 33)[0];  // :98-99: first CHARACTER of the number
            xseq += evs[e].cons;
            xqual.append(evs[e].cons.size(), nr.qraw[e]);
            nr.xoff[e + 1] = int64_t(xseq.size());
        }
        nr.hlen.resize(ne);
        nr.xf.resize(ne + 1);
        nr.xr.resize(ne + 1);
        std::vector<double> herr_k1(ne);
        std::vector<int32_t> xst(ne);
        int r = ioc_extract_minimizers(c, int32_t(ne), nr.xoff.data(), reinterpret_cast<const uint8_t*>(xseq.data()),
                                       reinterpret_cast<const uint8_t*>(xqual.data()), p->k, p->w, nr.hlen.data(), herr_k1.data(), nr.xf.data(),
                                       nr.xr.data(), xst.data());
        if (r != IOC_OK) return r;
        for (size_t e = 0; e < ne; ++e)
            if (xst[e] != 0) return ioc_fail(c, IOC_ERR_INPUT, "consensus with a non-ACGT base or an HPC length below 2k / w");
        const int64_t nmin = nr.xr[ne];
        nr.mv.resize(size_t(nmin) + 1);
        nr.mp.resize(size_t(nmin) + 1);
        if ((r = ioc_extracted_download(c, nr.mv.data(), nr.mp.data(), nmin)) != IOC_OK) return r;
        nr.hs.resize(xseq.size() + 1);
        std::vector<char> hq(xseq.size() + 1);
        return ioc_extracted_hpc_download(c, nr.hs.data(), hq.data(), int64_t(xseq.size()));
    }

    // Event ev's consensus — sequence e of nr — becomes the representative of its cluster: UpdateMinDB, the cluster's state, the
    // caller's record, ConsPurge.  di takes the cluster's old and new values.
    int install_representative(const PendingEvent& ev, const NewReps& nr, size_t e, DirtyIndex& di, std::vector<uint32_t>* upd_keys)
    {
        ClState& b = cl[size_t(ev.dc)];
        std::vector<uint32_t> nv(nr.mv.begin() + nr.xf[e], nr.mv.begin() + nr.xf[e + 1]);
        sorted_unique(nv);
        mdb.update(uint32_t(ev.dc), b.vals, nv, upd_keys);
        di.add_cluster(b.vals, nv);
        b.vals.swap(nv);
        b.raw_err = ev.raw_err;
        b.hpc_err = ev.hpc_err;  // consensus.cpp:121 — also when the 0.9999 branch (:112-117) fired
        b.raw = ev.cons;
        b.have_raw = true;
        b.seq_id = next_seq_id++;
        total.n_cons_invoked++;
        if (ops->rep_changed) {
            ioc_rep_record rec{};
            rec.raw_seq = ev.cons.data();
            rec.raw_len = int32_t(ev.cons.size());
            rec.raw_qual = nr.qraw[e];
            rec.raw_err = ev.raw_err;
            rec.raw_score = ev.raw_err * double(ev.cons.size());
            rec.hpc_seq = nr.hs.data() + nr.xoff[e];
            rec.hpc_len = int32_t(nr.hlen[e]);
            rec.hpc_err = ev.hpc_err;
            rec.fwd_min = nr.mv.data() + nr.xf[e];
            rec.fwd_pos = nr.mp.data() + nr.xf[e];
            rec.n_fwd = int32_t(nr.xf[e + 1] - nr.xf[e]);
            rec.rev_min = nr.mv.data() + nr.xr[e];
            rec.rev_pos = nr.mp.data() + nr.xr[e];
            rec.n_rev = int32_t(nr.xr[e + 1] - nr.xr[e]);
            rec.entry = ev.i;
            ops->rep_changed(ops->user, ev.dc, &rec);
        }
        const int gsz = ops->size(ops->user, 0, ev.dc);
        if (gsz > ca->cons_max_size) {  // ConsPurge, consensus.cpp:128-137
            if (ops->purge(ops->user, 0, ev.dc, ev.cons.data(), int(ev.cons.size()), unsigned(gsz)) < 0) return hook_fail(c, "purge");
        }
        return IOC_OK;
    }

    // Deferred mode, second half of a segment walked up to stop_x: consensus sequences, new representatives, verification, then
    // rollback or commit.  Entries [0, end_x) of the window stand.
    int finish_segment(Pass& ps, Segment& sg, int x_begin, int stop_x, int& end_x)
    {
        end_x = stop_x;
        if (sg.evs.empty()) return spec->commit(ops->user) < 0 ? hook_fail(c, "commit") : IOC_OK;
        double t1 = now_ms();
        n_spec_flushes++;
        if (spec->flush(ops->user, sg.evs[0].i) < 0) return hook_fail(c, "flush");
        ph[PH_FLUSH] += now_ms() - t1;
        int r;
        for (PendingEvent& ev : sg.evs)
            if ((r = take_consensus(spec->collect(ops->user, 0, ev.dc, ev.i, buf.data(), int(buf.size())), ev.cons)) != IOC_OK) return r;
        ph[PH_HOOKS] += now_ms() - t1;
        ph[PH_COLLECT] += now_ms() - t1;
        t1 = now_ms();
        NewReps nr;
        if ((r = new_representatives(sg.evs, nr)) != IOC_OK) return r;
        ph[PH_NEW_REP] += now_ms() - t1;
        t1 = now_ms();
        int violation = -1;
        if ((r = verify_segment(ps, sg, stop_x, nr, violation)) != IOC_OK) return r;
        ph[PH_VERIFY] += now_ms() - t1;
        const double t2 = now_ms();
        if (violation >= 0) {
            if ((r = rollback_from(ps, sg, violation)) != IOC_OK) return r;
            end_x = violation;
        } else if (spec->commit(ops->user) < 0) {
            return hook_fail(c, "commit");
        }
        ph[PH_NEW_REP] += now_ms() - t1;
        ph[PH_ROLLBACK] += now_ms() - t2;
        if (trace) fprintf(stderr, "[ioc]   deferred: %zu events in the segment, entries [%d, %d) stand\n", sg.evs.size(), ps.pos + x_begin, ps.pos + end_x);
        return IOC_OK;
    }

    // In the reference's order: finalize event e, then look again at the entries walked after it.  violation: the first window
    // entry from which everything is decided again (-1: the segment stands).
    int verify_segment(Pass& ps, Segment& sg, int stop_x, const NewReps& nr, int& violation)
    {
        sg.upd_keys.clear();
        size_t e = 0;
        const int x0 = sg.evs[0].x;
        for (int x = x0; x < stop_x && violation < 0; ++x) {
            // (an entry with an event of its own is looked at again like any other, before its event counts)
            if (x > x0 && force_rb && (++rb_counter % force_rb) == 0) violation = x;
            // it can see a NEW representative, or its hit order under the MinDB as the events before it leave it picks another candidate
            else if (x > x0 && ps.cls[size_t(x)] >= 0 && dirty_b.nslots && (can_see(dirty_b, ps, x) || !same_pick(ps, x))) violation = x;
            if (violation >= 0) break;
            if (e < sg.evs.size() && sg.evs[e].x == x) {
                if (const int r = install_representative(sg.evs[e], nr, e, dirty_b, &sg.upd_keys)) return r;
                ++e;
                if (dirty_b.full() && x + 1 < stop_x) violation = x + 1;  // too many changed clusters to keep checking: the pass ends here
            }
        }
        return IOC_OK;
    }

    // Undoes what the walk did for the window entries from `violation` on, newest first.
    int rollback_from(const Pass& ps, Segment& sg, int violation)
    {
        n_spec_rollbacks++;
        std::sort(sg.upd_keys.begin(), sg.upd_keys.end());
        for (size_t u = sg.journal.size(); u-- > 0;) {
            const Undo& un = sg.journal[u];
            if (un.x < violation) break;
            if (un.kind == 0) {
                total.n_gated--;
            } else if (un.kind == 1) {
                if (int32_t(cl.size()) - 1 != un.dc) return ioc_fail(c, IOC_ERR_STATE, "consensus rollback: cluster stack out of order");
                if (!mdb.undo_add(uint32_t(un.dc), cl.back().vals, un.key_was_new, sg.upd_keys))
                    return ioc_fail(c, IOC_ERR_STATE, "consensus rollback: MinDB out of order");
                cl.pop_back();
            } else {
                cl[size_t(un.dc)].size -= un.dsize;
                total.n_joined--;
            }
        }
        return spec->rollback(ops->user, ps.pos + violation) < 0 ? hook_fail(c, "rollback") : IOC_OK;
    }
};

}  // namespace

extern "C" {

int ioc_cluster_consensus(ioc_ctx* c, const ioc_params* p, const char* table_path, const ioc_left_view* left,
                          const ioc_batch_view* rb, const ioc_consensus_args* ca, const ioc_consensus_ops* ops,
                          int32_t* out_cls, int8_t* out_strand, ioc_cluster_stats* stats)
{
    if (!c || !p || !table_path || !rb || !ca || !ops || !out_cls || !out_strand) return IOC_ERR_ARG;
    if (!ops->create || !ops->size || !ops->add || !ops->consensus || !ops->purge)
        return ioc_fail(c, IOC_ERR_ARG, "consensus needs all five graph operations");
    const int n = rb->n;
    if (n < 0) return ioc_fail(c, IOC_ERR_ARG, "negative batch size");
    c->err.clear();
    if (!rb->raw_seq || !rb->raw_off)
        return ioc_fail(c, IOC_ERR_ARG, "consensus needs the raw sequences of the right batch (graph seeds and additions)");
    const bool aln_mode = p->mode == IOC_MODE_SAHLIN || p->mode == IOC_MODE_FURIOUS;
    if (left && left->n_keys < 0) return ioc_fail(c, IOC_ERR_ARG, "consensus takes the left MinDB as host arrays");
    if (aln_mode && left && left->n_clusters > 0 && (!left->rep_seq || !left->rep_off || !left->cls_raw_err))
        return ioc_fail(c, IOC_ERR_ARG, "sahlin/furious need the left representatives' sequences");

    // the windowed passes below read per-query state of every query of a pass: never sharded (ioc_set_shard)
    struct ShardOff {
        ioc_ctx* c;
        int world;
        explicit ShardOff(ioc_ctx* x) : c(x), world(x->shard_world) { c->shard_world = 1; }
        ~ShardOff() { c->shard_world = world; }
    } shard_off(c);
    struct DepSets {  // (run_pipeline leaves the order-dependent queries and their candidate sets while this driver runs)
        ioc_ctx* c;
        explicit DepSets(ioc_ctx* x) : c(x) { c->want_dep_sets = true; }
        ~DepSets() { c->want_dep_sets = false; }
    } dep_sets(c);
    c->aln_cache.clear();
    struct IdsGuard {
        ioc_ctx* c;
        ~IdsGuard()
        {
            c->aln_qid.clear();
            c->aln_lid.clear();
            c->aln_cache.clear();
        }
    } ids_guard{c};
    Driver d(c, p, table_path, rb, ca, ops, out_cls, out_strand);
    int r = d.load(left);
    if (r != IOC_OK) return r;

    // layout of the right batch's minimizer lists: the usual "all forward lists, then all reverse lists" lets a
    // suffix of the batch be handed over by pointer arithmetic
    bool blocked = n == 0 || rb->off_fwd[n] <= rb->off_rev[0];
    for (int i = 0; i < n && blocked; ++i) blocked = rb->off_fwd[i] <= rb->off_fwd[i + 1] && rb->off_rev[i] <= rb->off_rev[i + 1];
    if (!blocked)
        return ioc_fail(c, IOC_ERR_ARG, "consensus driver: minimizer lists must be laid out forward block, then reverse block");

    Pass ps;
    for (int pos = 0; pos < n;) {
        if ((r = d.run_pass(ps, pos)) != IOC_OK) return r;
        // Deferred mode walks a device pass in SEGMENTS: a segment ends — flush, new representatives, verification — where a pass
        // used to end, and also in front of an order-dependent entry met with consensus requests pending; in that case the walk
        // goes on from that entry on the same device decisions (dirty_b keeps every representative changed since the device pass:
        // an entry that can see one of them ends the device pass).
        d.dirty_b.reset();
        int x = 0;  // entries [0, x) of the window stand
        bool restarted = false;
        for (bool resume = true; resume;) {
            Segment sg;
            const int x_begin = x;
            const WalkEnd we = d.walk_segment(ps, sg, x_begin);
            if (we.rc != IOC_OK) return we.rc;
            x = we.x;
            if (d.spec && (r = d.finish_segment(ps, sg, x_begin, we.x, x)) != IOC_OK) return r;
            restarted = d.spec ? x < ps.m : we.how == Walk::Restart;
            resume = we.how == Walk::Resume && x == we.x && !d.dirty_b.full();  // (no violation: on from the order-dependent entry)
        }
        pos = ps.pos + x;
        d.next_window(restarted, x);
    }
    if (d.trace && d.spec)
        fprintf(stderr, "[ioc] deferred consensus: %lld events in %lld flushes, %lld rollbacks\n", (long long)d.n_spec_events,
                (long long)d.n_spec_flushes, (long long)d.n_spec_rollbacks);
    if (d.trace)
        fprintf(stderr, "[ioc] consensus phases: left view %.1f ms, device passes %.1f ms, graph hooks %.1f ms (flush %.1f, flush + collect %.1f), new representatives %.1f ms "
                        "(verification + UpdateMinDB %.1f, rollback / commit %.1f)\n",
                d.ph[PH_LEFT_VIEW], d.ph[PH_DEVICE], d.ph[PH_HOOKS], d.ph[PH_FLUSH], d.ph[PH_COLLECT], d.ph[PH_NEW_REP], d.ph[PH_VERIFY], d.ph[PH_ROLLBACK]);
    d.mdb.export_to(c);
    c->resolved = true;
    // the device state belongs to this driver's LAST windowed pass: a later ioc_set_aln_verdicts + ioc_resolve on the
    // context must not warm-start from it
    c->warm_first = -1;
    d.total.n_clusters = int64_t(d.cl.size());
    d.total.n_aln_invoked = 0;
    for (int i = 0; i < n; ++i) d.total.n_aln_invoked += d.aln_flag[size_t(i)];
    if (stats) *stats = d.total;
    return IOC_OK;
}

}  // extern "C"
