// workspace.hpp -- the per-(device, stream) workspace cache, defined once (mi_mcmc.hip) for the samplers there and the reducers of draws_api.hip.
// Kernels of one stream are ordered, so one buffer serves consecutive calls; it is
// reallocated (after a stream sync) only when a call needs more, and released by mi_mcmc_release_workspace().  A call holds
// the entry's mutex from ws_get() until its kernels are enqueued (WsLease), so a second host thread on the same stream can
// neither free nor regrow the buffer between "pointer handed out" and "kernel enqueued"; after that the stream orders them.
// (hipMallocAsync / hipFreeAsync pool memory was observed to hand the pack -> sample kernel pair of the logistic path
// buffers whose first blocks read back as zeros; a plain cached hipMalloc does not.)
// The mutex is not recursive: a function that may run under its caller's lease of the same stream (mi_mcmc_draw_stats under
// mi_mcmc_draw_stats_ranked) must not call ws_get().
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>

namespace mi {
namespace host {

struct WsEntry { void* p = nullptr; size_t cap = 0; std::mutex mu; };

struct WsLease {
    std::unique_lock<std::mutex> lk;
    void* p = nullptr;
    template <class T> T* as() const { return static_cast<T*>(p); }
};

int ws_get(hipStream_t st, size_t bytes, WsLease& lease);
// bytes the cache holds for (current device, st) right now
size_t ws_cached_bytes(hipStream_t st);
// frees the cached workspace of (current device, st); all_streams: every entry of the current device
int ws_release(hipStream_t st, bool all_streams, uint64_t* freed);

}  // namespace host
}  // namespace mi
