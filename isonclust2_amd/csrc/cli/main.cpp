// isONclust2-hip — the `isONclust2 sort | cluster | dump | info` command line on top of the MI355X path.
//
// Mirrors the sub-commands and flags of the reference (src/main.cpp:29-73, src/args.cpp) so that the
// external batch-and-merge pipeline (README.md:105-117) can call it unchanged; every hot-path
// computation goes through the C ABI of libisonclust2_hip.so (no CPU fallback: without a GPU the
// tool exits with an error).  Host code here is I/O and bookkeeping only: FASTQ parsing, the batching
// policy of `sort` (main.cpp:149-199), the member moves of `cluster` (cluster.cpp:177-261), the TSV /
// FASTQ writers of `dump` (output.cpp:151-275).
//
// This file: the dispatch, `info`, and the resident worker behind `cluster` ("serve").  The commands: sort.cpp, cluster.cpp,
// dump.cpp with reports.cpp and report_plan.cpp, selftest.cpp; what they share: common.hpp.
#include <dlfcn.h>
#include <fcntl.h>
#include <getopt.h>
#include <poll.h>
#include <sys/file.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/un.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "common.hpp"

using namespace cer;
using std::cerr;
using std::endl;
using std::string;

static const char* VERSION = "2.4-hip-r1";

// info (src/main.cpp:384-399)
static int main_info(int argc, char** argv)
{
    if (argc < 2 || string(argv[1]) == "-h") {
        cerr << "isONclust2-hip info batch.cer" << endl;
        exit(0);
    }
    Batch b;
    string err;
    if (!load_batch(b, argv[1], err)) die(err);
    cerr << "Loaded batch from " << argv[1] << ":" << endl;
    print_batch_info(b);
    return 0;
}

// ===================================================================================================
// serve: the resident worker behind `cluster`
//
// A one-shot `cluster` process on config 2's batch spends 0.2 s starting the HIP runtime (0.06 s on a quiet card: a KFD process
// created right after another one's exit first waits for that one's teardown — the steady state of a batch-and-merge
// pipeline), 0.04 - 0.1 s in first-use costs (code objects, first allocations) and 0.1 s leaving, for 0.03 - 0.06 s of kernels
// (profiles/r05_cli_breakdown.txt).  So `cluster` hands its job to a worker process that stays: the first call of a pipeline
// starts it (fork + exec of this binary, before anything here has touched the GPU), later calls find it warm.  The command line,
// the files and the messages are the one-shot command's: the client sends its arguments, its working directory, its
// IOC_* / ISONCLUST2_* environment and its own stdout / stderr descriptors (SCM_RIGHTS), the worker runs main_cluster there on its
// resident context and answers with the exit code.  A worker takes one job at a time; concurrent callers each get their own
// (slots, chosen by a file lock the caller holds for the length of its job), a worker leaves after ISONCLUST2_SERVE_IDLE_S
// seconds (default 15) without a job.  ISONCLUST2_SERVE=0, or any failure to reach or start a worker: the job runs in this
// process, as before.  `isONclust2-hip serve stop` ends the callers' idle workers.
// ===================================================================================================
namespace serve {

static const uint32_t MAGIC = 0x31435349u;  // "ISC1"

static string dir_path()
{
    const char* base = getenv("ISONCLUST2_SERVE_DIR");
    return base ? string(base) : "/tmp/isonclust2-hip-" + std::to_string(unsigned(getuid()));
}
static int device()
{
    const char* e = getenv("ISONCLUST2_DEVICE");
    return e ? atoi(e) : 0;
}
// (a worker of another build — the binary or the library rebuilt since it started — must not answer for this one: the names
// carry a stamp of both files, the old worker idles out)
static string build_stamp()
{
    static string stamp;
    if (!stamp.empty()) return stamp;
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](const char* path) {
        struct stat sb;
        if (stat(path, &sb) != 0) return;
        for (unsigned long long v : {(unsigned long long)sb.st_ino, (unsigned long long)sb.st_size, (unsigned long long)sb.st_mtim.tv_sec, (unsigned long long)sb.st_mtim.tv_nsec})
            h = (h ^ v) * 1099511628211ull;
    };
    mix("/proc/self/exe");
    Dl_info di;
    if (dladdr(reinterpret_cast<void*>(&ioc_ctx_create), &di) && di.dli_fname) mix(di.dli_fname);
    // (... nor a worker that sees other devices than the caller: the runtime reads these once, when the worker starts)
    for (const char* nm : {"HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "GPU_DEVICE_ORDINAL"}) {
        const char* v = getenv(nm);
        for (const char* q = v ? v : "\x01"; *q; ++q) h = (h ^ (unsigned long long)(unsigned char)*q) * 1099511628211ull;
        h = (h ^ 0xFFull) * 1099511628211ull;
    }
    char buf[20];
    snprintf(buf, sizeof(buf), "%08llx", h & 0xFFFFFFFFull);
    return stamp = buf;
}
static string slot_base(int slot) { return dir_path() + "/" + build_stamp() + "d" + std::to_string(device()) + "s" + std::to_string(slot); }

static bool write_all(int fd, const void* p, size_t n)
{
    const char* c = static_cast<const char*>(p);
    while (n) {
        const ssize_t w = ::send(fd, c, n, MSG_NOSIGNAL);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return false;
        c += w;
        n -= size_t(w);
    }
    return true;
}
static bool read_all(int fd, void* p, size_t n)
{
    char* c = static_cast<char*>(p);
    while (n) {
        const ssize_t r = ::recv(fd, c, n, 0);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        c += r;
        n -= size_t(r);
    }
    return true;
}
static void put_str(string& b, const string& s)
{
    const uint32_t n = uint32_t(s.size());
    b.append(reinterpret_cast<const char*>(&n), 4);
    b += s;
}

// ---- the worker ----
static int worker(int slot)
{
    const string base = slot_base(slot), sock = base + ".sock";
    // one worker per slot: the lock lives as long as this process
    const int lk = open((base + ".worker").c_str(), O_CREAT | O_RDWR | O_CLOEXEC, 0600);
    if (lk < 0) return 0;
    {   // (a caller probing whether a worker is alive holds this lock for an instant: try a few times before concluding that
        // another worker has the slot)
        int got = -1;
        for (int t = 0; t < 40 && got != 0; ++t) {
            got = flock(lk, LOCK_EX | LOCK_NB);
            if (got != 0) usleep(500);
        }
        if (got != 0) return 0;
    }
    const int ls = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    sockaddr_un sa{};
    sa.sun_family = AF_UNIX;
    if (ls < 0 || sock.size() >= sizeof(sa.sun_path)) return 1;
    memcpy(sa.sun_path, sock.c_str(), sock.size() + 1);
    (void)unlink(sock.c_str());
    if (bind(ls, reinterpret_cast<sockaddr*>(&sa), sizeof(sa)) != 0 || listen(ls, 4) != 0) return 1;
    double idle_s = 15.0;
    if (const char* e = getenv("ISONCLUST2_SERVE_IDLE_S")) idle_s = std::max(0.1, atof(e));
    g_served = true;
    std::vector<string> applied;  // environment names the last job set here
    // (what the process that happened to start this worker had in ITS environment is not the next caller's: a job runs under
    // the IOC_* / ISONCLUST2_* variables its own caller sends, nothing else of that kind)
    for (char** e = environ; e && *e; ++e)
        if ((strncmp(*e, "IOC_", 4) == 0 || strncmp(*e, "ISONCLUST2_", 11) == 0) && strncmp(*e, "ISONCLUST2_SERVE_", 17) != 0) {
            const char* eq = strchr(*e, '=');
            if (eq) applied.emplace_back(*e, size_t(eq - *e));
        }
    for (;;) {
        pollfd pf{ls, POLLIN, 0};
        const int pr = poll(&pf, 1, int(idle_s * 1000.0));
        if (pr < 0 && errno == EINTR) continue;
        if (pr <= 0) break;  // idle: leave
        const int cs = accept4(ls, nullptr, nullptr, SOCK_CLOEXEC);
        if (cs < 0) continue;
        // header + the caller's stdout / stderr
        uint32_t hdr[2] = {0, 0};
        int fds[2] = {-1, -1};
        {
            iovec io{hdr, sizeof(hdr)};
            alignas(cmsghdr) char cbuf[CMSG_SPACE(sizeof(fds))];
            msghdr mh{};
            mh.msg_iov = &io;
            mh.msg_iovlen = 1;
            mh.msg_control = cbuf;
            mh.msg_controllen = sizeof(cbuf);
            ssize_t r;
            do r = recvmsg(cs, &mh, MSG_CMSG_CLOEXEC); while (r < 0 && errno == EINTR);
            if (r == ssize_t(sizeof(hdr)))
                for (cmsghdr* cm = CMSG_FIRSTHDR(&mh); cm; cm = CMSG_NXTHDR(&mh, cm))
                    if (cm->cmsg_level == SOL_SOCKET && cm->cmsg_type == SCM_RIGHTS && cm->cmsg_len == CMSG_LEN(sizeof(fds))) memcpy(fds, CMSG_DATA(cm), sizeof(fds));
        }
        bool quit = false;
        int rc = 1;
        if (hdr[0] == MAGIC && hdr[1] == 0xFFFFFFFFu) {
            quit = true;
            rc = 0;
        } else if (hdr[0] == MAGIC && hdr[1] <= (64u << 20) && fds[0] >= 0 && fds[1] >= 0) {
            string body(hdr[1], '\0');
            if (read_all(cs, &body[0], body.size())) {
                std::vector<string> args, env;
                size_t at = 0;
                auto get = [&](std::vector<string>& dst) {
                    uint32_t cnt = 0;
                    if (at + 4 > body.size()) return false;
                    memcpy(&cnt, body.data() + at, 4);
                    at += 4;
                    for (uint32_t i = 0; i < cnt; ++i) {
                        uint32_t n = 0;
                        if (at + 4 > body.size()) return false;
                        memcpy(&n, body.data() + at, 4);
                        at += 4;
                        if (at + n > body.size()) return false;
                        dst.emplace_back(body.data() + at, n);
                        at += n;
                    }
                    return true;
                };
                uint32_t ncwd = 0;
                if (get(args) && get(env) && at + 4 <= body.size() && (memcpy(&ncwd, body.data() + at, 4), at + 4 + ncwd <= body.size()) &&
                    chdir(string(body.data() + at + 4, ncwd).c_str()) == 0) {
                    for (auto& nm : applied) unsetenv(nm.c_str());
                    applied.clear();
                    for (auto& kv : env) {
                        const size_t eq = kv.find('=');
                        if (eq == string::npos) continue;
                        setenv(kv.substr(0, eq).c_str(), kv.c_str() + eq + 1, 1);
                        applied.push_back(kv.substr(0, eq));
                    }
                    // the job writes where its caller would have
                    fflush(nullptr);
                    const int keep1 = dup(1), keep2 = dup(2);
                    dup2(fds[0], 1);
                    dup2(fds[1], 2);
                    std::vector<char*> av;
                    for (auto& a : args) av.push_back(&a[0]);
                    av.push_back(nullptr);
                    optind = 0;  // (glibc: scan from the start again)
                    VERBOSE = false;
                    try {
                        rc = main_cluster(int(args.size()), av.data());
                    } catch (const JobExit& e) {
                        rc = e.rc;
                    } catch (const std::exception& e) {
                        std::cerr << "isONclust2-hip: " << e.what() << std::endl;
                        rc = 1;
                    }
                    std::cout.flush();
                    std::cerr.flush();
                    fflush(nullptr);
                    dup2(keep1, 1);
                    dup2(keep2, 2);
                    close(keep1);
                    close(keep2);
                    (void)!chdir("/");  // (the caller's directory is the caller's again)
                }
            }
        }
        if (fds[0] >= 0) close(fds[0]);
        if (fds[1] >= 0) close(fds[1]);
        const int32_t out = rc;
        (void)write_all(cs, &out, 4);
        close(cs);
        if (quit) break;
    }
    (void)unlink(sock.c_str());
    close(ls);
    fflush(nullptr);
    _exit(0);  // (as the one-shot command: the driver takes the context back)
}

static int connect_to(const string& sock)
{
    const int fd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    sockaddr_un sa{};
    sa.sun_family = AF_UNIX;
    if (fd < 0 || sock.size() >= sizeof(sa.sun_path)) {
        if (fd >= 0) close(fd);
        return -1;
    }
    memcpy(sa.sun_path, sock.c_str(), sock.size() + 1);
    if (connect(fd, reinterpret_cast<sockaddr*>(&sa), sizeof(sa)) != 0) {
        close(fd);
        return -1;
    }
    return fd;
}

static bool worker_alive(const string& base)
{
    const int lk = open((base + ".worker").c_str(), O_CREAT | O_RDWR | O_CLOEXEC, 0600);
    if (lk < 0) return false;
    const bool alive = flock(lk, LOCK_EX | LOCK_NB) != 0;
    close(lk);  // (if we got the lock this gives it back)
    return alive;
}

static bool spawn_worker(int slot)
{
    char exe[4096];
    const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
    if (n <= 0) return false;
    exe[n] = 0;
    const pid_t pid = fork();  // (nothing in this process has touched the GPU: the HIP runtime starts lazily)
    if (pid < 0) return false;
    if (pid == 0) {
        if (fork() != 0) _exit(0);  // the worker is nobody's child
        setsid();
        const int dn = open("/dev/null", O_RDWR);
        const string logp = slot_base(slot) + ".log";
        const int lg = getenv("ISONCLUST2_SERVE_LOG") ? open(logp.c_str(), O_CREAT | O_WRONLY | O_APPEND, 0600) : -1;
        dup2(dn, 0);
        dup2(lg >= 0 ? lg : dn, 1);
        dup2(lg >= 0 ? lg : dn, 2);
        for (int fd = 3; fd < 256; ++fd) close(fd);
        const string sl = std::to_string(slot);
        execl(exe, exe, "serve", "worker", sl.c_str(), static_cast<char*>(nullptr));
        _exit(127);
    }
    int st = 0;
    (void)waitpid(pid, &st, 0);
    return true;
}

// Hands `cluster` (argv as main_cluster takes it) to a worker.  Returns the job's exit code, or -1 when no worker could be
// reached before anything was sent: the caller then runs the job itself.
static int client(int argc, char** argv)
{
    const char* on = getenv("ISONCLUST2_SERVE");
    if (on && atoi(on) == 0) return -1;
    // (the help text leaves through exit(): answered here)
    std::vector<string> args(argv, argv + argc);
    for (size_t i = 1; i < args.size(); ++i)
        if (args[i] == "-h" || args[i] == "--help") return -1;
    char cwd[4096];
    if (!getcwd(cwd, sizeof(cwd))) return -1;
    const string dir = dir_path();
    if (mkdir(dir.c_str(), 0700) != 0 && errno != EEXIST) return -1;
    struct stat sb;
    if (lstat(dir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode) || sb.st_uid != getuid() || (sb.st_mode & 077) != 0) return -1;
    int max_slots = 5;  // (a card takes few processes at once; each resident worker keeps its buffers)
    if (const char* e = getenv("ISONCLUST2_SERVE_SLOTS")) max_slots = std::max(1, std::min(32, atoi(e)));
    // a slot nobody is using: the caller's lock on it lasts for the job
    int slot = -1, lk = -1;
    for (int pass = 0; pass < 2 && slot < 0; ++pass)
        for (int i = 0; i < max_slots; ++i) {
            const int fd = open((slot_base(i) + ".lock").c_str(), O_CREAT | O_RDWR | O_CLOEXEC, 0600);
            if (fd < 0) return -1;
            // first pass: a free slot whose worker is warm; second pass: any free slot; failing that, wait for slot 0
            if (flock(fd, LOCK_EX | LOCK_NB) == 0 && (pass == 1 || worker_alive(slot_base(i)))) {
                slot = i;
                lk = fd;
                break;
            }
            close(fd);
        }
    if (slot < 0) {
        lk = open((slot_base(0) + ".lock").c_str(), O_CREAT | O_RDWR | O_CLOEXEC, 0600);
        if (lk < 0 || flock(lk, LOCK_EX) != 0) return -1;
        slot = 0;
    }
    const string base = slot_base(slot), sock = base + ".sock";
    if (sock.size() >= sizeof(sockaddr_un{}.sun_path)) {  // (a directory too deep for a socket's name: the job runs here)
        close(lk);
        return -1;
    }
    int cs = worker_alive(base) ? connect_to(sock) : -1;
    if (cs < 0) {
        if (!spawn_worker(slot)) {
            close(lk);
            return -1;
        }
        for (int tries = 0; tries < 5000 && cs < 0; ++tries) {  // (the worker binds its socket before it does anything else)
            cs = connect_to(sock);
            if (cs < 0) usleep(1000);
            if (cs < 0 && tries > 200 && !worker_alive(base)) break;  // (it could not start: no point in waiting)
        }
        if (cs < 0) {
            close(lk);
            return -1;
        }
    }
    string body;
    {
        const uint32_t na = uint32_t(args.size());
        body.append(reinterpret_cast<const char*>(&na), 4);
        for (auto& a : args) put_str(body, a);
        std::vector<string> env;
        for (char** e = environ; e && *e; ++e)
            if (strncmp(*e, "IOC_", 4) == 0 || strncmp(*e, "ISONCLUST2_", 11) == 0) env.emplace_back(*e);
        const uint32_t ne = uint32_t(env.size());
        body.append(reinterpret_cast<const char*>(&ne), 4);
        for (auto& e : env) put_str(body, e);
        put_str(body, cwd);  // relative paths mean what they mean to the caller
    }
    uint32_t hdr[2] = {MAGIC, uint32_t(body.size())};
    int fds[2] = {1, 2};
    iovec io{hdr, sizeof(hdr)};
    alignas(cmsghdr) char cbuf[CMSG_SPACE(sizeof(fds))];
    memset(cbuf, 0, sizeof(cbuf));
    msghdr mh{};
    mh.msg_iov = &io;
    mh.msg_iovlen = 1;
    mh.msg_control = cbuf;
    mh.msg_controllen = sizeof(cbuf);
    cmsghdr* cm = CMSG_FIRSTHDR(&mh);
    cm->cmsg_level = SOL_SOCKET;
    cm->cmsg_type = SCM_RIGHTS;
    cm->cmsg_len = CMSG_LEN(sizeof(fds));
    memcpy(CMSG_DATA(cm), fds, sizeof(fds));
    ssize_t w;
    do w = sendmsg(cs, &mh, MSG_NOSIGNAL); while (w < 0 && errno == EINTR);
    if (w != ssize_t(sizeof(hdr))) {
        close(cs);
        close(lk);
        return -1;
    }
    int32_t rc = 1;
    if (!write_all(cs, body.data(), body.size()) || !read_all(cs, &rc, 4)) {
        // the job was handed over and the worker is gone (a crash takes its context with it): say so, do not run it twice
        std::cerr << "isONclust2-hip: the resident worker ended before the job did (ISONCLUST2_SERVE=0 runs the job in the calling process)" << std::endl;
        rc = 1;
    }
    close(cs);
    close(lk);
    return rc;
}

static int stop_all()
{
    int stopped = 0;
    for (int i = 0; i < 32; ++i) {
        const string base = slot_base(i);
        if (!worker_alive(base)) continue;
        const int cs = connect_to(base + ".sock");
        if (cs < 0) continue;
        uint32_t hdr[2] = {MAGIC, 0xFFFFFFFFu};
        int32_t rc = 0;
        if (write_all(cs, hdr, sizeof(hdr)) && read_all(cs, &rc, 4)) ++stopped;
        close(cs);
        for (int t = 0; t < 2000 && worker_alive(base); ++t) usleep(1000);  // (its context is gone when this returns)
    }
    std::cerr << "isONclust2-hip: " << stopped << " worker(s) stopped" << std::endl;
    return 0;
}

}  // namespace serve

int main(int argc, char** argv)
{
    if (argc < 2) {
        cerr << "isONclust2-hip <sort|cluster|dump|info|version|help> ..." << endl;
        return 0;
    }
    const string cmd = argv[1];
    // The GPU commands leave through _exit once their files are closed and the streams flushed: the HIP runtime's exit handlers
    // (code objects unloaded, every allocation returned one by one) cost a one-shot process 50 - 100 ms for nothing — the driver
    // takes the process's memory back either way.  IOC_CLI_CLEAN_EXIT=1: the ordinary way out (profilers and sanitizers write their results from exit handlers).
    auto leave = [](int rc) {
        std::cout.flush();
        std::cerr.flush();
        fflush(nullptr);
        if (getenv("IOC_CLI_CLEAN_EXIT")) return rc;
        _exit(rc);
    };
    if (cmd == "sort") return leave(main_sort(argc - 1, argv + 1));
    if (cmd == "cluster") {
        const int served = serve::client(argc - 1, argv + 1);
        if (served >= 0) return served;
        return leave(main_cluster(argc - 1, argv + 1));
    }
    if (cmd == "serve") {
        const string what = argc > 2 ? argv[2] : "";
        if (what == "worker" && argc > 3) return serve::worker(atoi(argv[3]));
        if (what == "stop") return serve::stop_all();
        std::cerr << "isONclust2-hip serve stop    (workers are started by `cluster` itself; ISONCLUST2_SERVE=0 turns them off)" << endl;
        return 0;
    }
    if (cmd == "dump") return main_dump(argc - 1, argv + 1);
    if (cmd == "info") return main_info(argc - 1, argv + 1);
    if (cmd == "selftest") return main_selftest(argc - 1, argv + 1);
    if (cmd == "golden") {  // writes the golden batch of the byte-layout tests (host only)
        if (argc < 3) die("isONclust2-hip golden out.cer");
        Batch g;
        make_golden_batch(g);
        string err;
        if (!save_batch(g, argv[2], err)) die(err);
        return 0;
    }
    if (cmd == "version") {
        cerr << "isONclust2 version: " << VERSION << endl;
        return 0;
    }
    if (cmd == "help") {
        cerr << "isONclust2-hip: sort, cluster, dump, info, version, help — flags as in isONclust2 v2.4" << endl;
        return 0;
    }
    cerr << "Invalid command: " << cmd << endl;
    return 0;
}
