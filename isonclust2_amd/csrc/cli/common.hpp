// What every command of isONclust2-hip uses: the error exit, the served-job state, the context, the small file helpers and one
// copy of the helpers that `sort`, `cluster` and `dump` share.  The commands themselves: sort.cpp, cluster.cpp, dump.cpp (with
// reports.cpp), selftest.cpp; main.cpp dispatches and holds the resident worker.
#ifndef ISONCLUST2_CLI_COMMON_HPP
#define ISONCLUST2_CLI_COMMON_HPP
#include <algorithm>
#include <chrono>
#include <fstream>
#include <functional>
#include <string>

#include "cer.hpp"
#include "isonclust2_hip.h"

extern bool VERBOSE;

// A served job (see "serve" in main.cpp) must not take the resident process down with it: its error exits unwind to the server loop.
struct JobExit {
    int rc;
};
extern bool g_served;
extern ioc_ctx* g_srv_ctx;  // the resident process's context, made by its first job

[[noreturn]] void die(const std::string& m);
std::string table_path();
ioc_ctx* make_ctx();
void check(ioc_ctx* c, int rc, const char* what);
void create_outdir(const std::string& d);
void create_file(const std::string& p, std::ofstream& f);
void print_batch_info(const cer::Batch& b);
int parse_mode(const std::string& m);

int main_sort(int argc, char** argv);
int main_cluster(int argc, char** argv);
int main_dump(int argc, char** argv);
int main_selftest(int argc, char** argv);
void make_golden_batch(cer::Batch& g);

// A <-> T, C <-> G; every other byte stays what it is
struct Complement {
    char of[256];
    Complement()
    {
        for (int x = 0; x < 256; ++x) of[x] = char(x);
        of[int('A')] = 'T', of[int('C')] = 'G', of[int('G')] = 'C', of[int('T')] = 'A';
    }
    char operator()(char ch) const { return of[(unsigned char)ch]; }
};
inline const Complement complement;
inline std::string revcomp(std::string s)
{
    std::reverse(s.begin(), s.end());
    for (char& ch : s) ch = complement(ch);
    return s;
}

// The lines of a mapped text file.  line(): the next line [b, l) without its newline; false at the end of the file (std::getline's
// rules: a last line without a newline counts, an empty remainder does not).
struct LineCursor {
    const char* p;
    const char* const e;
    bool line(const char*& b, const char*& l);
};

// IOC_TRACE: "[ioc] <command>: <what>  <ms since the last lap>" on stderr
class Lap {
    const char* cmd_;
    std::chrono::steady_clock::time_point t_;

public:
    const bool on;
    explicit Lap(const char* cmd);
    void operator()(const char* what);
};

// min(cap, the host's cores), at least 1
unsigned host_threads(unsigned cap);
// fn(0) .. fn(nt - 1) side by side, joined; one thread's worth runs in the caller
void run_threads(unsigned nt, const std::function<void(unsigned)>& fn);

#endif
