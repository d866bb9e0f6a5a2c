#include "common.hpp"

#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <thread>
#include <vector>

using namespace cer;
using std::cerr;
using std::endl;
using std::string;

bool VERBOSE = false;
bool g_served = false;
ioc_ctx* g_srv_ctx = nullptr;

[[noreturn]] void die(const string& m)
{
    cerr << m << endl;
    if (g_served) throw JobExit{1};
    // (no unwinding: `sort` calls this from a batch-writer thread while others still run, and the reference's own error exits
    // leave through exit(1) with nothing left to flush)
    fflush(nullptr);
    _exit(1);
}

string table_path()
{
    if (const char* e = getenv("ISONCLUST2_TABLE")) return e;
    char buf[4096];
    ssize_t n = readlink("/proc/self/exe", buf, sizeof(buf) - 1);
    string exe = n > 0 ? string(buf, size_t(n)) : string(".");
    size_t p = exe.rfind('/');
    string dir = p == string::npos ? "." : exe.substr(0, p);
    return dir + "/../data/pmin_shared.bin";
}

ioc_ctx* make_ctx()
{
    ioc_ctx* c = nullptr;
    int dev = 0;
    if (const char* e = getenv("ISONCLUST2_DEVICE")) dev = atoi(e);
    int rc = ioc_ctx_create(dev, &c);
    if (rc != IOC_OK) die("No usable MI355X device (ioc_ctx_create failed with " + std::to_string(rc) + "); there is no CPU fallback.");
    return c;
}

void check(ioc_ctx* c, int rc, const char* what)
{
    if (rc < 0) die(string(what) + ": " + ioc_last_error(c));
}

static int dir_exists(const string& p)
{
    struct stat info;
    return stat(p.c_str(), &info) == 0 && (info.st_mode & S_IFDIR);
}
void create_outdir(const string& d)
{
    if (dir_exists(d)) {
        cerr << "Warning: reusing existing output directory: " << d << endl;
        return;
    }
    if (mkdir(d.c_str(), 0755) != 0) die("Failed to create output directory!");
}
void create_file(const string& p, std::ofstream& f)
{
    f.open(p);
    if (!f.is_open()) die("Failed to open " + p + "!");
}

void print_batch_info(const Batch& b)
{
    int ncls = 0, nnt = 0;
    for (auto& c : b.Cls)
        if (c && !c->empty() && c->at(0) && c->at(0)->RawSeq && c->at(0)->RawSeq->score > -1) {
            ncls++;
            if (c->size() > 2) nnt++;
        }
    cerr << "\tBatch number: " << b.BatchNr << endl;
    cerr << "\tBatch range: [" << b.BatchStart << "," << b.BatchEnd << "]" << endl;
    cerr << "\tDepth: " << b.Depth << endl;
    cerr << "\tNr sequences: " << b.BatchEnd - b.BatchStart + 1 << endl;
    cerr << "\tNr bases: " << b.BatchBases << endl;
    cerr << "\tNr clusters: " << ncls << endl;
    cerr << "\tNr nontrivial clusters: " << nnt << endl;
    cerr << "\tMinimizers in database: " << b.Db.size() << endl;
    size_t ng = 0;
    for (auto& g : b.ConsGs) ng += !g.empty();
    if (ng)  // (beyond the reference's lines: the one field of a .cer that is not exchangeable with the reference)
        cerr << "\tConsensus graphs: " << ng << " in this build's own format (the reference serializes spoa graphs; not interchangeable)" << endl;
}

int parse_mode(const string& m)
{
    if (m == "sahlin") return Sahlin;
    if (m == "fast") return Fast;
    if (m == "furious") return Furious;
    die("Illegal clustering mode: " + m);
}

bool LineCursor::line(const char*& b, const char*& l)
{
    if (p >= e) return false;
    const char* nl = static_cast<const char*>(memchr(p, '\n', size_t(e - p)));
    b = p;
    l = nl ? nl : e;
    p = nl ? nl + 1 : e;
    return true;
}

Lap::Lap(const char* cmd) : cmd_(cmd), t_(std::chrono::steady_clock::now()), on(getenv("IOC_TRACE") != nullptr) {}
void Lap::operator()(const char* what)
{
    if (!on) return;
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[ioc] %s: %-44s %9.1f ms\n", cmd_, what, std::chrono::duration<double, std::milli>(t1 - t_).count());
    t_ = t1;
}

unsigned host_threads(unsigned cap) { return std::max(1u, std::min(cap, std::thread::hardware_concurrency())); }

void run_threads(unsigned nt, const std::function<void(unsigned)>& fn)
{
    if (nt <= 1) {
        fn(0);
        return;
    }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(fn, t);
    for (auto& x : th) x.join();
}
