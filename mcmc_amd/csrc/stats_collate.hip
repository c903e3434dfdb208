// stats_collate.hip -- the multi-GPU helpers of the C ABI (shard arithmetic, RCCL all-gather of the kept draws, merge kernel) and the
// host layout converter.  The reducers over a draws slab are draws_api.hip and draw_stats.hip, where the converter's device form is as well.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <mutex>

#include "host_common.hpp"

using mi::host::fail;

namespace {

// all[k][j][chain0(r) + c] = rank_major[off(r) + (k d + j) n_local(r) + c]
__global__ __launch_bounds__(256) void merge_shards_kernel(const double* __restrict__ src, uint32_t world, uint64_t rows, uint64_t row0,
                                                          uint64_t C, double* __restrict__ dst)
{
    const uint64_t base = C / world, extra = C % world;
    const uint64_t row = row0 + blockIdx.y;                        // k d + j
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < C; c += (uint64_t)gridDim.x * blockDim.x) {
        // rank of global chain c and its position inside the shard
        const uint64_t cut = extra * (base + 1);
        const uint64_t r = (c < cut) ? c / (base + 1) : extra + (base ? (c - cut) / base : 0);
        const uint64_t c0 = r * base + (r < extra ? r : extra), nl = base + (r < extra ? 1 : 0);
        const uint64_t off = rows * c0;                            // shards before r hold rows * chain0(r) doubles in total
        dst[row * C + c] = src[off + row * nl + (c - c0)];
    }
}

struct Rccl {
    void* h = nullptr;
    int (*group_start)() = nullptr;
    int (*group_end)() = nullptr;
    int (*broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*allgather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*err)(int) = nullptr;
};
Rccl* rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"}) { r.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (r.h) break; }
        if (!r.h) return;
        r.group_start = reinterpret_cast<int (*)()>(dlsym(r.h, "ncclGroupStart"));
        r.group_end = reinterpret_cast<int (*)()>(dlsym(r.h, "ncclGroupEnd"));
        r.broadcast = reinterpret_cast<int (*)(const void*, void*, size_t, int, int, void*, hipStream_t)>(dlsym(r.h, "ncclBroadcast"));
        r.allgather = reinterpret_cast<int (*)(const void*, void*, size_t, int, void*, hipStream_t)>(dlsym(r.h, "ncclAllGather"));
        r.err = reinterpret_cast<const char* (*)(int)>(dlsym(r.h, "ncclGetErrorString"));
    });
    return (r.h && r.group_start && r.group_end && r.broadcast && r.allgather) ? &r : nullptr;
}

}  // namespace

extern "C" {

// ---- multi-GPU helpers of the C ABI (one process per GPU; mcmc_amd/dist.py is the torch.distributed form of the same thing)
void mi_mcmc_shard_bounds(uint64_t n_total, uint32_t world, uint32_t rank, uint64_t* chain0, uint64_t* n_local)
{
    // contiguous, balanced: the first (n % world) ranks get one extra chain
    const uint64_t base = world ? n_total / world : 0, extra = world ? n_total % world : 0;
    if (n_local) *n_local = base + (rank < extra ? 1 : 0);
    if (chain0) *chain0 = (uint64_t)rank * base + (rank < extra ? rank : extra);
}

int mi_mcmc_merge_shards(const double* rank_major, uint32_t world, uint64_t n_keep, uint64_t d, uint64_t C, double* all, void* stream)
{
    if (!rank_major || !all || world == 0) return fail(MI_ERR_BAD_ARG, "merge_shards: null buffer / empty world");
    const uint64_t rows = n_keep * d;
    if (rows == 0 || C == 0) return MI_OK;
    const unsigned gx = (unsigned)std::min<uint64_t>((C + 255) / 256, 4096);
    (void)hipGetLastError();
    for (uint64_t r0 = 0; r0 < rows; r0 += 65535) {        // grid.y limit
        const unsigned gy = (unsigned)std::min<uint64_t>(65535, rows - r0);
        hipLaunchKernelGGL(merge_shards_kernel, dim3(gx, gy), dim3(256), 0, static_cast<hipStream_t>(stream), rank_major, world, rows, r0, C, all);
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// ragged shards: one broadcast per rank into the rank-major staging buffer, grouped into one RCCL launch
int mi_mcmc_allgather_draws_ragged(void* comm, uint32_t world, uint32_t rank, const double* local, uint64_t n_keep, uint64_t d, uint64_t C,
                                   double* scratch, double* all, void* stream)
{
    if (!comm || !scratch || !all || world == 0 || rank >= world) return fail(MI_ERR_BAD_ARG, "allgather_draws: bad communicator / buffers / rank");
    Rccl* r = rccl();
    if (!r) return fail(MI_ERR_UNSUPPORTED, "allgather_draws: librccl.so could not be loaded");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t rows = n_keep * d;
    uint64_t c0 = 0, nl = 0;
    mi_mcmc_shard_bounds(C, world, rank, &c0, &nl);
    if (nl > 0 && !local) return fail(MI_ERR_BAD_ARG, "allgather_draws: local_draws is required for a non-empty shard");
    int e = r->group_start();
    for (uint32_t q = 0; q < world && e == 0; ++q) {
        uint64_t qc0 = 0, qn = 0;
        mi_mcmc_shard_bounds(C, world, q, &qc0, &qn);
        if (qn == 0) continue;
        // (sendbuff is read on the root only; the other ranks pass their receive slot, a valid device pointer, not NULL)
        double* slot = scratch + rows * qc0;
        e = r->broadcast(q == rank ? static_cast<const void*>(local) : static_cast<const void*>(slot), slot, (size_t)(rows * qn), 8 /* ncclDouble */, (int)q, comm, st);
    }
    const int e2 = r->group_end();
    if (e != 0 || e2 != 0) return fail(MI_ERR_HIP, "allgather_draws: RCCL: %s", r->err ? r->err(e ? e : e2) : "error");
    return mi_mcmc_merge_shards(scratch, world, n_keep, d, C, all, stream);
}

// north_star: "a single RCCL all-gather over xGMI to collate draws_out".  Equal shards (every BASELINE split: 65 536 / 8, 2^20 / 8) are
// exactly one ncclAllGather into the rank-major staging buffer, then the merge kernel puts every chain at its global index; ragged
// shards fall back to the grouped broadcasts above.
int mi_mcmc_allgather_draws(void* comm, uint32_t world, uint32_t rank, const double* local, uint64_t n_keep, uint64_t d, uint64_t C,
                            double* scratch, double* all, void* stream)
{
    if (!comm || !scratch || !all || world == 0 || rank >= world) return fail(MI_ERR_BAD_ARG, "allgather_draws: bad communicator / buffers / rank");
    if (C % world != 0 || C == 0) return mi_mcmc_allgather_draws_ragged(comm, world, rank, local, n_keep, d, C, scratch, all, stream);
    Rccl* r = rccl();
    if (!r) return fail(MI_ERR_UNSUPPORTED, "allgather_draws: librccl.so could not be loaded");
    if (!local) return fail(MI_ERR_BAD_ARG, "allgather_draws: local_draws is required for a non-empty shard");
    const uint64_t per = n_keep * d * (C / world);
    const int e = r->allgather(local, scratch, (size_t)per, 8 /* ncclDouble */, comm, static_cast<hipStream_t>(stream));
    if (e != 0) return fail(MI_ERR_HIP, "allgather_draws: RCCL: %s", r->err ? r->err(e) : "error");
    return mi_mcmc_merge_shards(scratch, world, n_keep, d, C, all, stream);
}

// ---- SURVEY 8(e)'s own receive layout: rank-major [G][n_keep][d][C / G], which equal shards fill with ONE ncclAllGather straight into
// the caller's buffer -- no staging buffer, no merge kernel, half the memory of mi_mcmc_allgather_draws (configs[4], n_keep = 8: 64 GiB
// + the 8 GiB local slab per GPU instead of 64 + 64 + 8).  Ragged shards: the packed form, shard r at offset rows * chain0(r) with its
// own row length n_local(r) (what mi_mcmc_merge_shards reads); one grouped broadcast per rank.
// row0 / n_keep_total: the slab is rows [row0, row0 + n_keep) of a run that keeps n_keep_total draws, gathered INTO the run's one
// rank-major buffer (per kept-draw slab, overlapped with the next trajectory: mi_mcmc_allgather_draws_begin below).  A partial slab
// is not contiguous on the receiving side across ranks, so it travels as one grouped broadcast per rank (one RCCL launch).
namespace {
int gather_rank_major(Rccl* r, void* comm, uint32_t world, uint32_t rank, const double* local, uint64_t n_keep, uint64_t d, uint64_t C,
                      uint64_t row0, uint64_t n_keep_total, double* all, hipStream_t st)
{
    uint64_t c0 = 0, nl = 0;
    mi_mcmc_shard_bounds(C, world, rank, &c0, &nl);
    if (nl > 0 && !local) return fail(MI_ERR_BAD_ARG, "allgather_draws: local_draws is required for a non-empty shard");
    if (C % world == 0 && C > 0 && row0 == 0 && n_keep == n_keep_total) {       // north_star's single all-gather
        const int e = r->allgather(local, all, (size_t)(n_keep * d * (C / world)), 8 /* ncclDouble */, comm, st);
        if (e != 0) return fail(MI_ERR_HIP, "allgather_draws: RCCL: %s", r->err ? r->err(e) : "error");
        return MI_OK;
    }
    int e = r->group_start();
    for (uint32_t q = 0; q < world && e == 0; ++q) {
        uint64_t qc0 = 0, qn = 0;
        mi_mcmc_shard_bounds(C, world, q, &qc0, &qn);
        if (qn == 0 || n_keep == 0) continue;
        double* slot = all + n_keep_total * d * qc0 + row0 * d * qn;             // shard q's block, its rows [row0, row0 + n_keep)
        e = r->broadcast(q == rank ? static_cast<const void*>(local) : static_cast<const void*>(slot), slot, (size_t)(n_keep * d * qn), 8, (int)q, comm, st);
    }
    const int e2 = r->group_end();
    if (e != 0 || e2 != 0) return fail(MI_ERR_HIP, "allgather_draws: RCCL: %s", r->err ? r->err(e ? e : e2) : "error");
    return MI_OK;
}

// one communication stream per device for the overlapped form: collectives of one communicator must be enqueued in the same order
// on every rank, which a single stream per device gives by construction
hipStream_t comm_stream(int dev)
{
    static std::mutex mu;
    static hipStream_t streams[64] = {};
    std::lock_guard<std::mutex> g(mu);
    if (dev < 0 || dev >= 64) return nullptr;
    if (!streams[dev] && hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking) != hipSuccess) streams[dev] = nullptr;
    return streams[dev];
}
}  // namespace

struct mi_collation { hipEvent_t done; };

int mi_mcmc_allgather_draws_rank_major(void* comm, uint32_t world, uint32_t rank, const double* local, uint64_t n_keep, uint64_t d, uint64_t C,
                                       double* all_rank_major, void* stream)
{
    if (!comm || !all_rank_major || world == 0 || rank >= world) return fail(MI_ERR_BAD_ARG, "allgather_draws: bad communicator / buffers / rank");
    Rccl* r = rccl();
    if (!r) return fail(MI_ERR_UNSUPPORTED, "allgather_draws: librccl.so could not be loaded");
    return gather_rank_major(r, comm, world, rank, local, n_keep, d, C, 0, n_keep, all_rank_major, static_cast<hipStream_t>(stream));
}

uint64_t mi_mcmc_rank_major_index(uint64_t C, uint32_t world, uint64_t n_keep, uint64_t d, uint64_t i, uint64_t j, uint64_t c)
{
    if (world == 0 || c >= C) return ~(uint64_t)0;
    const uint64_t base = C / world, extra = C % world, cut = extra * (base + 1);
    const uint64_t r = (c < cut) ? c / (base + 1) : extra + (base ? (c - cut) / base : 0);
    const uint64_t c0 = r * base + (r < extra ? r : extra), nl = base + (r < extra ? 1 : 0);
    return n_keep * d * c0 + (i * d + j) * nl + (c - c0);
}

int mi_mcmc_allgather_draws_begin(void* comm, uint32_t world, uint32_t rank, const double* local, uint64_t n_keep, uint64_t d, uint64_t C,
                                  uint64_t row0, uint64_t n_keep_total, double* all_rank_major, void* producer_stream, mi_collation** handle)
{
    if (!handle) return fail(MI_ERR_BAD_ARG, "allgather_draws_begin: null handle");
    *handle = nullptr;
    if (!comm || !all_rank_major || world == 0 || rank >= world || row0 + n_keep > n_keep_total)
        return fail(MI_ERR_BAD_ARG, "allgather_draws_begin: bad communicator / buffers / rank / row range");
    Rccl* r = rccl();
    if (!r) return fail(MI_ERR_UNSUPPORTED, "allgather_draws: librccl.so could not be loaded");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipStream_t cs = comm_stream(dev);
    if (!cs) return fail(MI_ERR_HIP, "allgather_draws_begin: no communication stream");
    hipEvent_t ready = nullptr, done = nullptr;
    // (every early return below releases what it created: no event outlives a failed call)
    auto try_hip = [&](hipError_t e, const char* what) -> int {
        if (e == hipSuccess) return MI_OK;
        if (ready) (void)hipEventDestroy(ready);
        if (done) (void)hipEventDestroy(done);
        return fail(MI_ERR_HIP, "allgather_draws_begin: %s: %s", what, hipGetErrorString(e));
    };
    int rc;
    if ((rc = try_hip(hipEventCreateWithFlags(&ready, hipEventDisableTiming), "event"))) return rc;
    if ((rc = try_hip(hipEventRecord(ready, static_cast<hipStream_t>(producer_stream)), "record"))) return rc;   // the slab is complete when the producer stream gets here
    if ((rc = try_hip(hipStreamWaitEvent(cs, ready, 0), "wait"))) return rc;
    (void)hipEventDestroy(ready);                                                  // (released once the wait has consumed it)
    ready = nullptr;
    rc = gather_rank_major(r, comm, world, rank, local, n_keep, d, C, row0, n_keep_total, all_rank_major, cs);
    if (rc) return rc;
    if ((rc = try_hip(hipEventCreateWithFlags(&done, hipEventDisableTiming), "event"))) return rc;
    if ((rc = try_hip(hipEventRecord(done, cs), "record"))) return rc;
    *handle = new mi_collation{done};
    return MI_OK;
}

int mi_mcmc_allgather_draws_wait(mi_collation* handle, void* consumer_stream, int block_host)
{
    if (!handle) return fail(MI_ERR_BAD_ARG, "allgather_draws_wait: null handle");
    hipError_t e = block_host ? hipEventSynchronize(handle->done) : hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), handle->done, 0);
    (void)hipEventDestroy(handle->done);
    delete handle;
    if (e != hipSuccess) return fail(MI_ERR_HIP, "allgather_draws_wait: %s", hipGetErrorString(e));
    return MI_OK;
}

int mi_mcmc_draws_to_chain_major(const double* kdc, uint64_t n_keep, uint64_t d, uint64_t C, double* out)
{
    if (!kdc || !out) return fail(MI_ERR_BAD_ARG, "null buffer");
    // host arrays: blocked over chains so that both sides stay in cache (the device form, in draw_stats.hip, is the one for slabs in HBM)
    constexpr uint64_t CB = 64;
    for (uint64_t c0 = 0; c0 < C; c0 += CB)
        for (uint64_t j = 0; j < d; ++j)
            for (uint64_t i = 0; i < n_keep; ++i) {
                const double* src = kdc + (i * d + j) * C;
                const uint64_t c1 = std::min(C, c0 + CB);
                for (uint64_t c = c0; c < c1; ++c) out[(c * d + j) * n_keep + i] = src[c];
            }
    return MI_OK;
}

}  // extern "C"
