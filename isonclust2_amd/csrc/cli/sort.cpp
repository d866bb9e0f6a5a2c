// sort  (src/main.cpp:75-202): FASTQ -> quality scores on the device -> sorted FASTQ, index, scores -> the batch files
#include <getopt.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <future>
#include <iostream>
#include <mutex>
#include <vector>

#include "common.hpp"

using namespace cer;
using std::cerr;
using std::endl;
using std::string;

static CmdArgs parse_sort_options(int argc, char** argv)
{
    static const struct option lo[] = {
        {"version", no_argument, 0, 'V'}, {"verbose", no_argument, 0, 'v'}, {"debug", no_argument, 0, 'd'},
        {"mode", required_argument, 0, 'x'}, {"help", no_argument, 0, 'h'}, {"kmer-size", required_argument, 0, 'k'},
        {"window-size", required_argument, 0, 'w'}, {"min-shared", required_argument, 0, 'm'},
        {"mapped-threshold", required_argument, 0, 'r'}, {"aligned-threshold", required_argument, 0, 'a'},
        {"min-fraction", required_argument, 0, 'f'}, {"min-prob-no-hits", required_argument, 0, 'p'},
        {"min-qual", required_argument, 0, 'q'}, {"min-cls-size", required_argument, 0, 'F'},
        {"low-cons-size", required_argument, 0, 'g'}, {"max-cons-size", required_argument, 0, 'c'},
        {"cons-period", required_argument, 0, 'P'}, {"outfolder", required_argument, 0, 'o'},
        {"batch-size", required_argument, 0, 'B'}, {"batch-max-seq", required_argument, 0, 'M'}, {0, 0, 0, 0}};
    CmdArgs a;
    int o;
    while ((o = getopt_long(argc, argv, "k:w:dhvo:m:r:a:f:p:q:B:x:g:c:M:P:F:", lo, nullptr)) != -1) {
        switch (o) {
            case 'k': a.KmerSize = atoi(optarg); break;
            case 'w': a.WindowSize = atoi(optarg); break;
            case 'm': a.MinShared = atoi(optarg); break;
            case 'r': a.MappedThreshold = atof(optarg); break;
            case 'a': a.AlignedThreshold = atof(optarg); break;
            case 'f': a.MinFraction = atof(optarg); break;
            case 'p': a.MinProbNoHits = atof(optarg); break;
            case 'q': a.MinQual = atof(optarg); break;
            case 'B': a.BatchSize = atoi(optarg); break;
            case 'M': a.BatchMaxSeq = atoi(optarg); break;
            case 'P': a.ConsPeriod = atoi(optarg); break;
            case 'g': a.ConsMinSize = atoi(optarg); break;
            case 'c': a.ConsMaxSize = atoi(optarg); break;
            case 'F': a.MinClsSize = atoi(optarg); break;
            case 'o': a.BatchOutFolder = optarg; break;
            case 'v': a.Verbose = true; break;
            case 'd': a.Debug = true; break;
            case 'x': a.Mode = parse_mode(optarg); break;
            case 'h': cerr << "isONclust2-hip sort [options] reads.fastq  (flags as `isONclust2 sort`)" << endl; exit(0);
            default: break;
        }
    }
    // src/args.cpp:135-148
    if (a.KmerSize < 10 || a.KmerSize > 31) die("Invalid kmer size (must be in [10,31])!");
    if (a.KmerSize > a.WindowSize) die("The window size must be larger than or equal to the kmer size!");
    if (optind >= argc) die("No input fastq specified!");
    a.InFastq = argv[optind];
    return a;
}

// (parsed out of a read-only mapping: a read's bases and qualities are views of it — nothing of an 8 GB file is copied)
static std::vector<Seq> parse_fastq(const MappedFile& fqmap)
{
    std::vector<Seq> reads;
    LineCursor in{fqmap.data, fqmap.data + fqmap.size};
    const char *hb, *he, *sb, *se, *pb, *pe, *qb, *qe;
    while (in.line(hb, he)) {
        if (he == hb) continue;
        const string h(hb, size_t(he - hb));
        if (!in.line(sb, se) || !in.line(pb, pe) || !in.line(qb, qe)) die("Truncated fastq record: " + h);
        if (hb[0] != '@' || se - sb != qe - qb) die("Malformed fastq record: " + h);
        Seq r;
        const size_t sp = h.find_first_of(" \t");
        r.name = h.substr(1, sp == string::npos ? string::npos : sp - 1);
        r.seq = Bytes(sb, size_t(se - sb), fqmap.keep);
        r.qual = Bytes(qb, size_t(qe - qb), fqmap.keep);
        reads.push_back(std::move(r));
    }
    return reads;
}

// FillQualScores on the device, SortByQualScores on the host
static void score_and_sort(ioc_ctx* c, int kmer_size, std::vector<Seq>& reads, Lap& lap)
{
    const int n = int(reads.size());
    std::vector<int64_t> offs(static_cast<size_t>(n) + 1, 0);
    for (int i = 0; i < n; ++i) offs[size_t(i) + 1] = offs[size_t(i)] + int64_t(reads[size_t(i)].qual.size());
    {
        std::shared_ptr<void> qual_mem = huge_alloc(static_cast<size_t>(offs[size_t(n)]) + 1);
        uint8_t* const qual = static_cast<uint8_t*>(qual_mem.get());
        const unsigned nt = host_threads(8);
        run_threads(nt, [&](unsigned t0) {
            for (int i = int(t0); i < n; i += int(nt)) memcpy(qual + offs[size_t(i)], reads[size_t(i)].qual.data(), reads[size_t(i)].qual.size());
        });
        std::vector<double> score(static_cast<size_t>(n)), err(static_cast<size_t>(n));
        check(c, ioc_qual_scores(c, n, offs.data(), qual, kmer_size, score.data(), err.data()), "quality scores");
        for (int i = 0; i < n; ++i) {
            reads[size_t(i)].score = score[size_t(i)];
            reads[size_t(i)].errorRate = err[size_t(i)];
        }
    }
    lap("quality scores (GPU)");
    std::stable_sort(reads.begin(), reads.end(), [](const Seq& x, const Seq& y) { return x.score > y.score; });
    lap("stable sort");
}

// sorted_reads.fastq, its two indices and scores.tsv
static void write_sorted_files(const string& folder, const std::vector<Seq>& reads)
{
    std::ofstream tsv, sc;
    const string sorted = folder + "/sorted_reads.fastq";
    GatherFile fq;  // (the bases and qualities go from the input's mapping to the page cache in one gather per 1024 pieces)
    if (!fq.open(sorted)) die("Failed to open " + sorted + "!");
    create_file(folder + "/sorted_reads_idx.tsv", tsv);
    tsv << "Id\tPos" << endl;
    unsigned long long seek = 0;
    for (auto& r : reads) {
        if (r.score < 0) continue;
        tsv << r.name << "\t" << seek << "\n";  // (the same bytes as endl, without a write() per read)
        fq.put("@", 1);
        fq.put(r.name.data(), r.name.size());
        fq.put("\n", 1);
        fq.put(r.seq.data(), r.seq.size());
        fq.put("\n+\n", 3);
        fq.put(r.qual.data(), r.qual.size());
        fq.put("\n", 1);
        seek += r.name.size() + r.seq.size() + r.qual.size() + 6;
    }
    if (!fq.close()) die("Failed to write " + sorted + "!");
    save_sorted_idx(sorted, folder + "/sorted_reads_idx.cer");
    create_file(folder + "/scores.tsv", sc);
    for (auto& r : reads) sc << r.name << "\t" << r.score << "\n";
}

struct Range {
    int start, end;
    unsigned long bases;
    int nr;
};

// main.cpp:149-199: a batch ends after BatchSize kilobases or BatchMaxSeq reads
static std::vector<Range> plan_batches(const CmdArgs& a, const std::vector<Seq>& reads)
{
    const int n = int(reads.size());
    std::vector<Range> ranges;
    unsigned long batch_bases = 0;
    int batch_seqs = 0, nr_batches = 0, batch_start = 0;
    for (int i = 0; i < n; ++i) {
        batch_bases += reads[size_t(i)].seq.size();
        batch_seqs++;
        if (a.BatchSize > 0 && (batch_bases > (unsigned long)(a.BatchSize) * 1000ul || (a.BatchMaxSeq > 0 && batch_seqs >= a.BatchMaxSeq))) {
            ranges.push_back(Range{batch_start, i, batch_bases, nr_batches});
            batch_bases = 0;
            batch_seqs = 0;
            batch_start = i + 1;
            nr_batches++;
        }
    }
    if (batch_start < n) ranges.push_back(Range{batch_start, n - 1, batch_bases, nr_batches});
    return ranges;
}

// What the batch writers share.  The batches are independent once the reads are sorted: the extraction of a batch runs on the
// one context (a mutex around the three calls), the assembly of its records and its file are built by worker threads side by side
// (IOC_SORT_THREADS, default 6: the 64 batches of a 2 M-read file took 29 s one after the other).
struct SortJob {
    const CmdArgs& a;
    ioc_ctx* c;
    std::vector<Seq>& reads;  // (a read too short for its batch gets score -1 here)
    const string batch_dir;
    std::mutex ctx_mu, log_mu;
    std::atomic<long long> us_dev{0}, us_asm{0}, us_save{0};  // (IOC_TRACE: summed over the batches' threads)
};

static long long us_now()
{
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static void write_batch(SortJob& job, const Range& range)
{
    const CmdArgs& a = job.a;
    ioc_ctx* const c = job.c;
    std::vector<Seq>& reads = job.reads;
    const int start = range.start, nr = range.nr;
    // (every large buffer of a batch comes in huge pages — 0.9 GB of first touches per 31 250-read batch otherwise, six threads at
    // once — and the records are views of them: nothing is copied per read, cer.hpp)
    const int m = range.end - start + 1;
    std::vector<int64_t> bo(static_cast<size_t>(m) + 1, 0);
    for (int i = 0; i < m; ++i) bo[size_t(i) + 1] = bo[size_t(i)] + int64_t(reads[size_t(start + i)].seq.size());
    const size_t nb = static_cast<size_t>(bo[size_t(m)]);
    std::shared_ptr<void> seq_mem = huge_alloc(nb + 1), qual_mem = huge_alloc(nb + 1);
    uint8_t* const seq = static_cast<uint8_t*>(seq_mem.get());
    uint8_t* const qual = static_cast<uint8_t*>(qual_mem.get());
    for (int i = 0; i < m; ++i) {
        memcpy(seq + bo[size_t(i)], reads[size_t(start + i)].seq.data(), reads[size_t(start + i)].seq.size());
        memcpy(qual + bo[size_t(i)], reads[size_t(start + i)].qual.data(), reads[size_t(start + i)].qual.size());
    }
    std::vector<uint32_t> hlen(static_cast<size_t>(m));
    std::vector<double> herr(static_cast<size_t>(m));
    std::vector<int64_t> of(static_cast<size_t>(m) + 1), orv(static_cast<size_t>(m) + 1);
    std::vector<int32_t> status(static_cast<size_t>(m));
    std::shared_ptr<void> hs_mem = huge_alloc(nb + 1), hq_mem = huge_alloc(nb + 1);
    char* const hs = static_cast<char*>(hs_mem.get());
    char* const hq = static_cast<char*>(hq_mem.get());
    std::unique_lock<std::mutex> dev(job.ctx_mu);  // ---- the one context: extraction and its downloads, one batch at a time ----
    const long long t_dev = us_now();
    check(c, ioc_extract_minimizers(c, m, bo.data(), seq, qual, a.KmerSize, a.WindowSize, hlen.data(),
                                    herr.data(), of.data(), orv.data(), status.data()), "minimizer extraction");
    const int64_t tot = orv[size_t(m)];
    std::shared_ptr<void> mv_mem = huge_alloc((static_cast<size_t>(tot) + 1) * 4), mp_mem = huge_alloc((static_cast<size_t>(tot) + 1) * 4);
    uint32_t* const mv = static_cast<uint32_t*>(mv_mem.get());
    uint32_t* const mp = static_cast<uint32_t*>(mp_mem.get());
    check(c, ioc_extracted_download(c, mv, mp, tot + 1), "minimizer download");
    check(c, ioc_extracted_hpc_download(c, hs, hq, int64_t(nb + 1)), "hpc download");
    dev.unlock();
    const long long t_asm = us_now();
    job.us_dev += t_asm - t_dev;
    seq_mem.reset();
    qual_mem.reset();
    // the minimizers as the records hold them (Min, Pos, Index): one array for the batch
    std::shared_ptr<void> aos_mem = huge_alloc((static_cast<size_t>(tot) + 1) * sizeof(Minimizer));
    Minimizer* const aos = static_cast<Minimizer*>(aos_mem.get());
    auto fill = [&](Span<Minimizer>& out, int64_t b0, int64_t e0) {
        for (int64_t t = b0; t < e0; ++t) aos[size_t(t)] = Minimizer{mv[size_t(t)], mp[size_t(t)], uint32_t(t - b0)};
        out = Span<Minimizer>(aos + b0, size_t(e0 - b0), aos_mem);
    };
    Batch b;
    b.Cls.resize(size_t(m));
    for (int i = 0; i < m; ++i) {
        Seq& r = reads[size_t(start + i)];
        auto cl = std::make_shared<Cluster>();
        auto ps = std::make_shared<ProcSeq>();
        ps->Id = r.name;
        const bool lowq = (-10 * log10(r.errorRate)) <= a.MinQual;            // qualscore.cpp:56
        const bool lenok = r.seq.size() > size_t(2 * a.KmerSize) || r.seq.size() >= size_t(a.WindowSize);
        if (status[size_t(i)] == 2) die("Invalid base encountered in read " + r.name);   // RevComp throws
        if (lowq) {
            // placeholder {nullptr, nullptr, {}, {}, 0, name}
        } else if (!lenok || status[size_t(i)] == 1) {
            r.score = -1.0;  // qualscore.cpp:67, :91 (the reference's raw-only branch is unreachable without a crash)
        } else {
            ps->RawSeq.reset(new Seq(r));
            ps->HpcSeq.reset(new Seq);
            ps->HpcSeq->name = r.name;
            ps->HpcSeq->seq = Bytes(hs + bo[size_t(i)], hlen[size_t(i)], hs_mem);
            ps->HpcSeq->qual = Bytes(hq + bo[size_t(i)], hlen[size_t(i)], hq_mem);
            ps->HpcSeq->score = r.score;
            ps->HpcSeq->errorRate = herr[size_t(i)];
            fill(ps->Mins, of[size_t(i)], of[size_t(i) + 1]);
            fill(ps->RevMins, orv[size_t(i)], orv[size_t(i) + 1]);
            ps->MatchStrand = 1;
        }
        cl->push_back(ps);
        b.Cls[size_t(i)] = cl;
    }
    b.NrCls = m;
    b.BatchStart = uint64_t(start);
    b.BatchEnd = uint64_t(range.end);
    b.Depth = -1;
    b.BatchNr = nr;
    b.BatchBases = range.bases;
    b.SortArgs = a;
    string err;
    const long long t_save = us_now();
    job.us_asm += t_save - t_asm;
    if (!save_batch(b, job.batch_dir + "/isONbatch_" + std::to_string(nr) + ".cer", err)) die(err);
    job.us_save += us_now() - t_save;
    if (VERBOSE) {
        std::lock_guard<std::mutex> lk(job.log_mu);
        cerr << "\tWritten batch " << nr << " with " << m << " sequences and " << int(double(range.bases) / 1000.0) << " kilobases." << endl;
    }
}

int main_sort(int argc, char** argv)
{
    const CmdArgs a = parse_sort_options(argc, argv);
    VERBOSE = a.Verbose;
    Lap lap("sort");
    // ---- FASTQ (whole file in RAM, like bioparser Parse(-1), main.cpp:109-112) ----
    auto ctx_future = std::async(std::launch::async, [] { return make_ctx(); });  // (the runtime starts beside the parsing)
    MappedFile fqmap;
    {
        string merr;
        if (!map_file(a.InFastq, fqmap, merr)) die("Failed to open " + a.InFastq + "!");
    }
    std::vector<Seq> reads = parse_fastq(fqmap);
    if (VERBOSE) cerr << "Parsed " << reads.size() << " sequences." << endl;
    lap("fastq parsed");

    ioc_ctx* c = ctx_future.get();
    lap("context (started beside the parsing)");
    score_and_sort(c, a.KmerSize, reads, lap);

    SortJob job{a, c, reads, a.BatchOutFolder + "/batches"};
    create_outdir(a.BatchOutFolder);
    create_outdir(job.batch_dir);
    write_sorted_files(a.BatchOutFolder, reads);
    lap("sorted fastq, index, scores written");

    // ---- batches (main.cpp:149-199) ----
    const std::vector<Range> ranges = plan_batches(a, reads);
    {
        int nt = 6;
        if (const char* e = getenv("IOC_SORT_THREADS")) nt = std::max(1, atoi(e));
        nt = std::min<int>(nt, int(ranges.size()));
        std::atomic<size_t> next{0};
        run_threads(unsigned(std::max(nt, 0)), [&](unsigned) {
            for (size_t x = next.fetch_add(1); x < ranges.size(); x = next.fetch_add(1)) write_batch(job, ranges[x]);
        });
    }
    lap("batches extracted and written");
    if (lap.on)
        fprintf(stderr, "[ioc] sort:   of it, summed over the batches: device section (one at a time) %.1f ms, record assembly %.1f ms, file %.1f ms\n",
                job.us_dev.load() / 1e3, job.us_asm.load() / 1e3, job.us_save.load() / 1e3);
    ioc_ctx_destroy(c);
    return 0;
}
