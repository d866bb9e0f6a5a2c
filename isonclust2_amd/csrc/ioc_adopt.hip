// ioc_adopt.hip — ioc_left_adopt: the clustering just resolved becomes the context's left state without leaving the device.
//
// What ioc_index_export followed by ioc_left_load would carry over the host is already in HBM after the export's kernels:
// the final MinDB as CSR (ascending keys, offsets, renumbered ascending posting lists; index_export_compute, ioc_capi.cpp) and
// the final id of every query that opened a cluster (b_exp_cid).  What is left to make is what ioc_left_load forms on one
// host core, posting by posting:
//   * the err cell of every cluster: the old left clusters keep theirs, a new cluster has its query's;
//   * the transposed MinDB (cluster -> its sorted distinct values, the membership sets of getMappedRatio).  No transposition
//     is needed: an old left cluster is in exactly the lists it was in before (the export keeps every left posting), so its
//     set is its present segment, and a query that opened a cluster is in the lists of its distinct forward values, which the
//     index build keeps sorted per query (dvals).  The new sets are a segmented gather of segments that exist.
// Every output word has one writer that is a function of the input alone: the result is the same from run to run.
// Host traffic: the `valid` bytes and the sizes of the export, and the L + 1 set offsets h_lset_off mirrors.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "ioc_internal.h"
#include "ioc_kernels.h"

namespace {

// Per old left cluster and per query that opened a cluster: the length of its value set, its err cell and — for the
// queries — which query a new cluster came from (src_q[final id - L]).
__global__ void __launch_bounds__(256)
k_adopt_heads(int32_t L, int32_t n, const int64_t* __restrict__ old_set_off, const uint8_t* __restrict__ old_err,
              const int32_t* __restrict__ cid, const uint32_t* __restrict__ dcount, const uint8_t* __restrict__ q_err,
              uint32_t* __restrict__ len, uint8_t* __restrict__ new_err, int32_t* __restrict__ src_q)
{
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t < L) {
        len[t] = uint32_t(old_set_off[t + 1] - old_set_off[t]);
        new_err[t] = old_err[t];
    }
    if (t < n) {
        const int32_t id = cid[t];
        if (id >= 0) {  // (final ids are distinct and >= L: one writer per cell)
            len[id] = dcount[t];
            new_err[id] = q_err[t];
            src_q[id - L] = int32_t(t);
        }
    }
}

// One wave per cluster: its offset as int64 and its value set, copied from the segment it already has (64 consecutive
// words per step in and out).
__global__ void __launch_bounds__(256)
k_adopt_sets(int32_t L, int32_t L_new, const uint32_t* __restrict__ off32, const int64_t* __restrict__ old_set_off,
             const uint32_t* __restrict__ old_set_val, const int32_t* __restrict__ src_q, const int64_t* __restrict__ doff,
             const uint32_t* __restrict__ dvals, int64_t* __restrict__ out_off, uint32_t* __restrict__ out_val, uint32_t out_cap)
{
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t w0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6, nw = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t cl = w0; cl <= L_new; cl += nw) {
        const uint32_t o = off32[cl];
        if (lane == 0) out_off[cl] = int64_t(o);
        if (cl == L_new) break;
        const uint32_t m = off32[cl + 1] - o;
        const uint32_t* src = cl < L ? old_set_val + old_set_off[cl] : dvals + doff[src_q[cl - L]];
        for (uint32_t e = lane; e < m; e += 64)
            if (o + e < out_cap) out_val[o + e] = src[e];  // (sets that do not add up to the MinDB's postings are refused on the host)
    }
}

}  // namespace

extern "C" {

int ioc_left_adopt(ioc_ctx* c, int32_t* n_clusters)
{
    if (!c) return IOC_ERR_ARG;
    IOC_CHK(c, hipSetDevice(c->device));
    if (!c->resolved || !c->built) return ioc_fail(c, IOC_ERR_STATE, "ioc_left_adopt: no resolved pass to adopt (ioc_resolve first)");
    // (the consensus driver ends with the MinDB it kept on the host, UpdateMinDB's edits included: the device holds its last
    // window only)
    if (c->exp_valid && !c->exp_dev && !(getenv("IOC_EXPORT_HOST_ORDER") && atoi(getenv("IOC_EXPORT_HOST_ORDER")) != 0))
        return ioc_fail(c, IOC_ERR_STATE, "ioc_left_adopt: the last call's MinDB is held by the host (ioc_cluster_consensus)");
    IOC_TRY(ioc_wait_uploads(c, 2));
    IOC_TRY(ioc_export_on_device(c));
    hipStream_t s = c->stream;
    const int32_t L = c->L, n = c->n, Ln = c->exp_clusters;
    const int64_t nrows = int64_t(c->exp_nrows), total = int64_t(c->exp_total);
    if (Ln < L || Ln - L > n) return ioc_fail(c, IOC_ERR_STATE, "ioc_left_adopt: cluster count of the export out of range");
    if (total >= (int64_t(1) << 31)) return ioc_fail(c, IOC_ERR_CAPACITY, "more than 2^31 index postings");
    // work: [len: Ln + 1][off32: Ln + 1][src_q: n + 1][scan scratch]
    auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
    const size_t o_len = 0, o_off = o_len + up((size_t(Ln) + 1) * 4), o_src = o_off + up((size_t(Ln) + 1) * 4),
                 o_scan = o_src + up((size_t(n) + 1) * 4), work_bytes = o_scan + ((size_t(Ln) + 1) / 256 + 1024) * 4 * 2;
    IOC_TRY(ioc_reserve(c, c->b_adopt_work, work_bytes));
    IOC_TRY(ioc_reserve(c, c->b_alt_err, size_t(Ln)));
    IOC_TRY(ioc_reserve(c, c->b_alt_keys, size_t(nrows) * 4));
    IOC_TRY(ioc_reserve(c, c->b_alt_offs, size_t(nrows + 1) * 8));
    IOC_TRY(ioc_reserve(c, c->b_alt_set_off, (size_t(Ln) + 1) * 8));
    IOC_TRY(ioc_reserve(c, c->b_alt_set_val, size_t(total) * 4));
    IOC_TRY(ioc_reserve(c, c->b_lslot, size_t(nrows) * 4));
    uint8_t* wk = c->b_adopt_work.as<uint8_t>();
    uint32_t* d_len = reinterpret_cast<uint32_t*>(wk + o_len);
    uint32_t* d_off32 = reinterpret_cast<uint32_t*>(wk + o_off);
    int32_t* d_src = reinterpret_cast<int32_t*>(wk + o_src);
    std::vector<int64_t> soff(size_t(Ln) + 1, 0);
    if (Ln > 0) {
        const int64_t span = std::max<int64_t>(L, n);
        hipLaunchKernelGGL(k_adopt_heads, dim3(uint32_t((span + 255) / 256)), dim3(256), 0, s, L, n, c->b_lset_off.as<int64_t>(),
                           c->b_left_err.as<uint8_t>(), c->b_exp_cid.as<int32_t>(), c->b_dcount.as<uint32_t>(), c->d_err_cell, d_len,
                           c->b_alt_err.as<uint8_t>(), d_src);
        IOC_CHK(c, hipGetLastError());
        IOC_CHK(c, iock_exclusive_scan(s, d_len, Ln, d_off32, reinterpret_cast<uint32_t*>(wk + o_scan), 0u));
        const uint32_t waves = uint32_t(std::min<int64_t>(int64_t(Ln) + 1, 8192));
        hipLaunchKernelGGL(k_adopt_sets, dim3((waves + 3) / 4), dim3(256), 0, s, L, Ln, d_off32, c->b_lset_off.as<int64_t>(),
                           c->b_lset_val.as<uint32_t>(), d_src, c->b_doff.as<int64_t>(), c->b_dvals.as<uint32_t>(),
                           c->b_alt_set_off.as<int64_t>(), c->b_alt_set_val.as<uint32_t>(), uint32_t(total));
        IOC_CHK(c, hipGetLastError());
        IOC_CHK(c, hipMemcpyAsync(soff.data(), c->b_alt_set_off.p, (size_t(Ln) + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    const uint8_t* ex = c->b_exp_work.as<uint8_t>();
    if (nrows) IOC_CHK(c, hipMemcpyAsync(c->b_alt_keys.p, ex + c->exp_o_keys, size_t(nrows) * 4, hipMemcpyDeviceToDevice, s));
    if (nrows)
        IOC_CHK(c, hipMemcpyAsync(c->b_alt_offs.p, ex + c->exp_o_offs, size_t(nrows + 1) * 8, hipMemcpyDeviceToDevice, s));
    else
        IOC_CHK(c, hipMemsetAsync(c->b_alt_offs.p, 0, 8, s));
    IOC_CHK(c, hipStreamSynchronize(s));
    // every posting (key, cluster) of the MinDB is one value of that cluster's set
    if (soff[size_t(Ln)] != total)
        return ioc_fail(c, IOC_ERR_STATE, "ioc_left_adopt: the value sets hold " + std::to_string(soff[size_t(Ln)]) + " values, the MinDB " +
                                              std::to_string(total) + " postings");
    // ---- swap the new state in (the stream is idle) ----
    std::swap(c->b_left_err, c->b_alt_err);
    std::swap(c->b_lkeys, c->b_alt_keys);
    std::swap(c->b_loffs, c->b_alt_offs);
    std::swap(c->b_lset_off, c->b_alt_set_off);
    std::swap(c->b_lset_val, c->b_alt_set_val);
    if (total > 0)
        std::swap(c->b_lpost, c->b_exp_out);  // (the export's compact postings ARE the new lists)
    else
        IOC_TRY(ioc_reserve(c, c->b_lpost, 0));
    c->h_lset_off.swap(soff);
    c->L = Ln;
    c->n_left_keys = nrows;
    c->n_left_post = total;
    c->exp_dev = c->exp_valid = false;
    c->built = c->scored = c->resolved = false;  // the queries are released: the next pass builds its index against the new left state
    if (n_clusters) *n_clusters = Ln;
    return IOC_OK;
}

}  // extern "C"
