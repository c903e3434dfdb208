// host_common.hpp -- shared by the host-side translation units of the C ABI (mi_mcmc.hip: the samplers; mass_adapt.hip: the mass adaptations
// above them, over sampler_host.hpp; callback_host.hip: the host-callback routes; draws_api.hip and draw_stats.hip: the reducers over a draws
// slab; stats_collate.hip: multi-GPU collation and the host layout converter; probes.hip: diagnostics): the error channel (status code + thread-local message behind mi_mcmc_last_error), the
// device probe, the RAII device buffer and the staging of a host slab.  The workspace cache the samplers and the reducers share is workspace.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/mi_mcmc.h"

namespace mi {
namespace host {

std::string& last_error();                         // thread-local, defined in mi_mcmc.hip
std::string& last_kernel();                        // thread-local: what mi_mcmc_last_kernel() returns

inline int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}

// The device probe of an entry point, placed after its argument checks (they need no device): MI_OK with HIP's sticky status cleared -- a stale
// non-fatal status of the caller's own HIP use (e.g. hipErrorNotReady of an event query) is not ours --, or MI_ERR_NO_DEVICE
inline int need_device()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MI_ERR_NO_DEVICE, "no HIP device visible: the engine has no CPU path");
    (void)hipGetLastError();
    return MI_OK;
}

// RAII device buffer
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// One chain of `algo` (0 hmc, 1 mala, 2 nuts, 3 rwmh, 4 rmhmc) on the literal kernel with HOST callbacks as target (mi_mcmc.hip; the
// kernel asks the host through a pinned mailbox): bounds, precond_mat / cov_mat, any max_tree_depth <= 30.  tensor_fn: rmhmc only.
int literal_run_callback(const char* who, int algo, const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel, void* target_data,
                         mi_tensor_cb tensor_fn, void* tensor_data, const mi_settings* settings, double* draws_out,
                         uint64_t* n_accept_draws, double* step_size_out);

}  // namespace host
}  // namespace mi

#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return ::mi::host::fail(e_ == hipErrorOutOfMemory ? MI_ERR_OOM : MI_ERR_HIP, "%s failed: %s", \
                                    #expr, hipGetErrorString(e_));                                       \
    } while (0)

namespace mi {
namespace host {

// The slab of a call on the device: the caller's own pointer, or for a host slab a fresh buffer (staged owns it; not the workspace) with the copy
// enqueued on st.  The buffer dies with the DevBuf, so the caller synchronises the stream before it returns.
inline int stage_slab(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, hipStream_t st, DevBuf& staged, const double** x)
{
    *x = draws_kdc;
    if (mem != MI_MEM_HOST) return MI_OK;
    HIP_TRY(staged.alloc(n_keep * d * n_chains * 8));
    HIP_TRY(hipMemcpyAsync(staged.p, draws_kdc, n_keep * d * n_chains * 8, hipMemcpyHostToDevice, st));
    *x = staged.as<double>();
    return MI_OK;
}

}  // namespace host
}  // namespace mi
