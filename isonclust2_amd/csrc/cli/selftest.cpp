// selftest, golden: the .cer reader and writer against a synthetic batch and a byte image spelled out by hand (host only)
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "common.hpp"

using namespace cer;
using std::cerr;
using std::endl;
using std::string;

// the tiny batch whose byte image is spelled out twice: in main_selftest below and — independently, from SURVEY.md App. B and
// the serialize() member orders — in tests/test_cer_golden.py (`isONclust2-hip golden <path>` writes it)
void make_golden_batch(Batch& g)
{
    g.BatchNr = 1;
    g.BatchStart = 2;
    g.BatchEnd = 3;
    g.BatchBases = 4;
    g.TotalReads = 5;
    g.NrCls = 1;
    g.SortArgs.InFastq = "a";
    g.SortArgs.BatchOutFolder = "b";
    g.SortArgs.Mode = Fast;
    g.LeftLeaf = "L";
    g.RightLeaf = "";
    g.Depth = -1;
    g.Db = {{9u, {0u}}};
    auto cl = std::make_shared<Cluster>();
    auto ps = std::make_shared<ProcSeq>();
    ps->RawSeq.reset(new Seq{"n", "AC", "II", 1.5, 0.25});
    ps->Mins = std::vector<Minimizer>{{1, 2, 3}};
    ps->MatchStrand = 1;
    ps->Id = "i";
    cl->push_back(ps);
    g.Cls.push_back(cl);
    g.NrConsGs = 1;
}

// .cer round trip on a synthetic batch (host only; used by the CPU test-suite)
int main_selftest(int argc, char** argv)
{
    const string path = argc > 1 ? argv[1] : "/tmp/isonclust2_selftest.cer";
    Batch b;
    b.BatchNr = 3;
    b.BatchStart = 10;
    b.BatchEnd = 12;
    b.BatchBases = 12345;
    b.NrCls = 3;
    b.Depth = 1;
    b.SortArgs.KmerSize = 13;
    b.SortArgs.WindowSize = 20;
    b.SortArgs.Mode = Fast;
    b.SortArgs.InFastq = "reads.fq";
    b.LeftLeaf = "a.cer";
    b.RightLeaf = "";
    b.Db = {{7u, {0u, 2u}}, {0xFFFFFFFFu, {1u}}, {99u, {}}};
    for (int c = 0; c < 3; ++c) {
        auto cl = std::make_shared<Cluster>();
        for (int m = 0; m <= c; ++m) {
            auto ps = std::make_shared<ProcSeq>();
            ps->Id = "r" + std::to_string(c) + "_" + std::to_string(m);
            ps->MatchStrand = m % 2 ? -1 : 1;
            if (m == 0) {
                ps->RawSeq.reset(new Seq{ps->Id, "ACGTACGT", "IIIIIIII", 7.5, 0.01});
                ps->HpcSeq.reset(new Seq{ps->Id, "ACGT", "IIII", 7.5, 0.02});
                ps->Mins = std::vector<Minimizer>{{1, 0, 0}, {5, 3, 1}};
                ps->RevMins = std::vector<Minimizer>{{3, 6, 0}};
            }
            cl->push_back(ps);
        }
        b.Cls.push_back(cl);
    }
    b.Cls.push_back(nullptr);
    b.NrConsGs = 3;
    string err;
    if (!save_batch(b, path, err)) die(err);
    Batch r;
    if (!load_batch(r, path, err)) die(err);
    bool ok = r.BatchNr == 3 && r.BatchStart == 10 && r.BatchEnd == 12 && r.BatchBases == 12345 && r.NrCls == 3 && r.Depth == 1 &&
              r.SortArgs.KmerSize == 13 && r.SortArgs.WindowSize == 20 && r.SortArgs.Mode == Fast && r.SortArgs.InFastq == "reads.fq" &&
              r.SortArgs.MinFraction == 0.8 && r.LeftLeaf == "a.cer" && r.Db.size() == 3 && r.Db[0].first == 7u &&
              r.Db[0].second == std::vector<uint32_t>({0u, 2u}) && r.Db[2].first == 0xFFFFFFFFu && r.Cls.size() == 4 && !r.Cls[3] &&
              r.NrConsGs == 3;
    for (int c = 0; ok && c < 3; ++c) {
        ok = r.Cls[size_t(c)] && int(r.Cls[size_t(c)]->size()) == c + 1;
        for (int m = 0; ok && m <= c; ++m) {
            auto& x = (*r.Cls[size_t(c)])[size_t(m)];
            auto& y = (*b.Cls[size_t(c)])[size_t(m)];
            ok = x->Id == y->Id && x->MatchStrand == y->MatchStrand && bool(x->RawSeq) == bool(y->RawSeq) &&
                 x->Mins.size() == y->Mins.size();
            if (ok && x->RawSeq)
                ok = x->RawSeq->seq == "ACGTACGT" && x->HpcSeq->errorRate == 0.02 && x->Mins[1].Pos == 3 && x->RevMins[0].Min == 3;
        }
    }
    // a truncated file must be rejected, not crash
    {
        std::ifstream in(path, std::ios::binary);
        string all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        std::ofstream out(path + ".trunc", std::ios::binary);
        out.write(all.data(), std::streamsize(all.size() / 2));
        out.close();
        Batch t;
        ok = ok && !load_batch(t, path + ".trunc", err);
        remove((path + ".trunc").c_str());
    }
    // every prefix of the file, a byte flipped at every offset, and crafted 64-bit counts (which must not wrap the
    // bounds checks) are rejected or loaded, never a crash: run under ASan / UBSan by tools/run_sanitizers.sh
    {
        std::ifstream in(path, std::ios::binary);
        const string all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        auto try_load = [&](const string& bytes) {
            std::ofstream out(path + ".var", std::ios::binary);
            out.write(bytes.data(), std::streamsize(bytes.size()));
            out.close();
            Batch t;
            string e2;
            return load_batch(t, path + ".var", e2);
        };
        for (size_t cut = 0; ok && cut < all.size(); ++cut) ok = !try_load(all.substr(0, cut));
        size_t loaded = 0;
        for (size_t at = 0; at < all.size(); ++at) {
            string v = all;
            v[at] = char(v[at] ^ 0xFF);
            loaded += try_load(v);
        }
        const uint64_t huge[3] = {0x4000000000000001ull, 0xFFFFFFFFFFFFFFFFull, 0x1555555555555556ull};  // x 4 and x 12 wrap
        for (size_t at = 0; ok && at + 8 <= all.size(); ++at)
            for (uint64_t h : huge) {
                string v = all;
                memcpy(&v[at], &h, 8);
                (void)try_load(v);
            }
        remove((path + ".var").c_str());
        cerr << "selftest: " << all.size() << " prefixes rejected, " << loaded << " single-byte variants still loadable" << endl;
    }
    // byte-level image of a minimal batch with consensus off, spelled out field by field under cereal's binary
    // conventions (cereal itself is absent from the reference tree: layout unverified against a
    // reference-written file, pinned here against silent drift)
    {
        Batch g;
        make_golden_batch(g);
        string want;
        auto p32 = [&](int32_t v) { want.append(reinterpret_cast<const char*>(&v), 4); };
        auto pu32 = [&](uint32_t v) { want.append(reinterpret_cast<const char*>(&v), 4); };
        auto p64 = [&](uint64_t v) { want.append(reinterpret_cast<const char*>(&v), 8); };
        auto pf = [&](double v) { want.append(reinterpret_cast<const char*>(&v), 8); };
        auto pstr = [&](const string& x) { p64(x.size()); want += x; };
        p32(1); p64(2); p64(3); p64(4); p32(5); p32(1);                                   // BatchNr .. NrCls
        want.push_back(0); want.push_back(0); pstr("a");                                    // Verbose, Debug, InFastq
        for (int32_t v : {11, 50000, 30000, 15, 5, 50, -150, 500, 3}) p32(v);               // KmerSize .. MinClsSize
        for (double v : {7.0, 0.65, 0.2, 0.8, 0.1}) pf(v);                                  // MinQual .. MinProbNoHits
        pstr("b"); p32(Fast);                                                               // BatchOutFolder, Mode
        pstr("L"); pstr(""); p32(-1);                                                       // LeftLeaf, RightLeaf, Depth
        p64(1); pu32(9); p64(1); pu32(0);                                                   // MinDB: 1 key -> 1 posting
        p64(1); pu32(0x80000001u); p64(1); pu32(0x80000002u);                               // Cls: shared_ptr ids, first occurrence
        want.push_back(1); pstr("n"); pstr("AC"); pstr("II"); pf(1.5); pf(0.25);            // RawSeq (valid)
        want.push_back(0);                                                                  // HpcSeq (null)
        p64(1); pu32(1); pu32(2); pu32(3); p64(0); p32(1); pstr("i");                        // Mins, RevMins, MatchStrand, Id
        p64(1); want.push_back(0);                                                          // ConsGs: one null graph
        if (!save_batch(g, path, err)) die(err);
        std::ifstream in(path, std::ios::binary);
        const string got((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (got != want) {
            cerr << "selftest: byte image differs from the spelled-out layout (" << got.size() << " vs " << want.size() << " bytes)" << endl;
            ok = false;
        }
        // a non-null graph that is not this build's blob is refused with a message, not read as garbage
        string v = want;
        v.back() = 1;
        p64(8);
        v.append(want.end() - 8, want.end());
        v += "SPOAGRPH";
        {
            std::ofstream out(path, std::ios::binary);
            out.write(v.data(), std::streamsize(v.size()));
        }
        Batch t;
        string e2;
        if (load_batch(t, path, e2) || e2.find("not in this build's format") == string::npos) {
            cerr << "selftest: foreign graph blob not refused: " << e2 << endl;
            ok = false;
        }
        // ... and so is a graph of the builds before the edge weights changed (IOCPOA1)
        v.replace(v.size() - 8, 8, string("IOCPOA1\0", 8));
        {
            std::ofstream out(path, std::ios::binary);
            out.write(v.data(), std::streamsize(v.size()));
        }
        if (load_batch(t, path, e2) || e2.find("earlier build") == string::npos) {
            cerr << "selftest: graph blob of an earlier build not refused: " << e2 << endl;
            ok = false;
        }
    }
    remove(path.c_str());
    cerr << (ok ? "selftest ok" : "selftest FAILED") << endl;
    return ok ? 0 : 1;
}
