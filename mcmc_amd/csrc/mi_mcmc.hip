// mi_mcmc.hip -- C ABI (include/mi_mcmc.h) of the MI355X many-chain HMC / MALA / NUTS engine.
// Host side of the boundary: validates the POD mirrors of algo_settings_t, stages targets and
// chain state in HBM, launches the gfx950 kernels.  No CPU fallback: anything the device path
// does not implement returns MI_ERR_UNSUPPORTED.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mi_mcmc.h"
#include "host_common.hpp"
#include "sampler_host.hpp"
#include "workspace.hpp"
#include "host_linalg.hpp"
#include "det_math.hpp"
#include "hmc_dense.hpp"
#include "nuts_dense.hpp"
#include "nuts_tile.hpp"
#include "nuts_async.hpp"
#include "mala_dense.hpp"
#include "rwmh_dense.hpp"
#define MI_DE_PARAMS_ONLY
#include "de.hpp"
#define MI_AEES_PARAMS_ONLY
#include "aees.hpp"
#include "hmc_diag.hpp"
#include "logistic_launch.hpp"
#include "launchers.hpp"
#include "gemm_samplers.hpp"
#include "small_samplers.hpp"
#include "literal_host.hpp"
#include "settings_host.hpp"
#include "tile_samplers.hpp"

// round time of the few-chain launch shapes of the plain HMC kernel relative to the default (two waves per SIMD), d = 128
#ifndef MI_HMC_COST_1WAVE
#define MI_HMC_COST_1WAVE 0.535       // 27.1 ms against 50.8 ms per round (tools/hmc_shapes.py)
#define MI_HMC_COST_SPLIT2 0.287      // 14.55 ms
#define MI_HMC_COST_SPLIT4X2 0.278    // 14.12 ms
#define MI_HMC_COST_SPLIT4 0.153      // 7.78 ms
#endif

namespace mi {
namespace host {
std::string& last_error() { thread_local std::string e; return e; }
std::string& last_kernel() { thread_local std::string k; return k; }
int device_inverse(const double* A, size_t d, double* Ainv);                 // linalg_device.hip
int device_cholesky_lower(const double* A, size_t d, double* L);

// the per-(device, stream) workspace cache (workspace.hpp says what it is): its one definition
static std::mutex g_ws_mu;
static std::map<std::pair<int, hipStream_t>, std::unique_ptr<WsEntry>> g_ws;

int ws_get(hipStream_t st, size_t bytes, WsLease& lease)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    WsEntry* w = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        std::unique_ptr<WsEntry>& slot = g_ws[std::make_pair(dev, st)];
        if (!slot) slot.reset(new WsEntry);
        w = slot.get();
    }
    lease.lk = std::unique_lock<std::mutex>(w->mu);
    if (w->cap < bytes) {
        if (w->p) { HIP_TRY(hipStreamSynchronize(st)); HIP_TRY(hipFree(w->p)); w->p = nullptr; w->cap = 0; }
        HIP_TRY(hipMalloc(&w->p, bytes));
        w->cap = bytes;
    }
    lease.p = w->p;
    return MI_OK;
}

size_t ws_cached_bytes(hipStream_t st)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lk(g_ws_mu);
    auto it = g_ws.find(std::make_pair(dev, st));
    return (it == g_ws.end() || !it->second) ? 0 : it->second->cap;
}

int ws_release(hipStream_t st, bool all_streams, uint64_t* freed)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::vector<WsEntry*> victims;
    {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        for (auto& kv : g_ws)
            if (kv.first.first == dev && (all_streams || kv.first.second == st)) victims.push_back(kv.second.get());
    }
    uint64_t total = 0;
    for (WsEntry* w : victims) {
        std::lock_guard<std::mutex> lk(w->mu);
        if (!w->p) continue;
        HIP_TRY(all_streams ? hipDeviceSynchronize() : hipStreamSynchronize(st));
        HIP_TRY(hipFree(w->p));
        total += w->cap;
        w->p = nullptr; w->cap = 0;
    }
    if (freed) *freed = total;
    return MI_OK;
}
}  // namespace host
namespace {
// INV / CHOL_LOWER of a dense precond_mat with d >= 64 run on the device (host_linalg.hpp: same operations per element, same bits)
const bool g_linalg_installed = [] {
    LinalgAccel& a = linalg_accel();
    a.inverse = host::device_inverse;
    a.cholesky_lower = host::device_cholesky_lower;
    return true;
}();
}  // namespace
void note_kernel(const char* fmt, ...)
{
    char buf[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    host::last_kernel() = buf;
}
// The test hook's cap on the persistent grids is read ONCE per sampler call (snapshot_grid_cap, at the first thing every route does) into a
// thread-local: the workspace of a call is sized and its kernel launched from the same value even if another thread moves the cap in between
// (sized with one grid, launched with a larger one, the kernel would write point records out of bounds).
namespace { std::atomic<uint64_t> g_test_grid_cap{0}; thread_local uint64_t t_grid_cap = 0; }
uint64_t test_grid_cap() { return t_grid_cap; }
uint64_t test_grid_cap_now() { return g_test_grid_cap.load(std::memory_order_relaxed); }
namespace { void snapshot_grid_cap() { t_grid_cap = g_test_grid_cap.load(std::memory_order_relaxed); } }
}  // namespace mi

// test hook, declared in mi_mcmc_probes.h (not in the product header): see launch_common.hpp
extern "C" void mi_mcmc_test_set_grid_cap(uint32_t max_workgroups) { mi::g_test_grid_cap.store(max_workgroups, std::memory_order_relaxed); }
// test hook, declared in mi_mcmc_probes.h: the staging budget of the device INV / CHOL_LOWER (host_linalg.hpp)
extern "C" void mi_mcmc_test_set_linalg_stage_bytes(uint32_t bytes) { linalg_set_stage_bytes(bytes); }
extern "C" uint64_t mi_mcmc_test_linalg_computed(void) { return linalg_accel().n_computed.load(std::memory_order_relaxed); }
extern "C" uint64_t mi_mcmc_test_linalg_computed_on_device(void) { return linalg_accel().n_on_device.load(std::memory_order_relaxed); }
// test hooks, declared in mi_mcmc_probes.h: the workspace budget of nuts on the matrix-product route (run_gemm_nuts), the ranges it has run, and the host
// arithmetic of its routing (plain functions: they need no device)
namespace { std::atomic<uint64_t> g_gemm_nuts_ws_bytes{0}, g_gemm_nuts_ranges{0}, g_gemm_nuts_ticks{0}, g_gemm_nuts_points{0}, g_gemm_nuts_slots{0}; }
extern "C" void mi_mcmc_test_set_gemm_nuts_ws_bytes(uint64_t bytes) { g_gemm_nuts_ws_bytes.store(bytes, std::memory_order_relaxed); }
extern "C" uint64_t mi_mcmc_test_gemm_nuts_ranges(void) { return g_gemm_nuts_ranges.load(std::memory_order_relaxed); }
extern "C" void mi_mcmc_test_gemm_nuts_last_ticks(uint64_t* ticks, uint64_t* busy_slots, uint64_t* slots)
{
    if (ticks) *ticks = g_gemm_nuts_ticks.load(std::memory_order_relaxed);
    if (busy_slots) *busy_slots = g_gemm_nuts_points.load(std::memory_order_relaxed);
    if (slots) *slots = g_gemm_nuts_slots.load(std::memory_order_relaxed);
}
extern "C" uint64_t mi_mcmc_test_gemm_nuts_tick_ceiling(uint32_t max_tree_depth, uint64_t n_draws, int search) { return mi::gemm::gemm_nuts_tick_ceiling(max_tree_depth, n_draws, search != 0); }
extern "C" uint64_t mi_mcmc_test_gemm_nuts_chain_bytes(uint32_t d, uint32_t n_rows, uint32_t max_tree_depth) { return mi::gemm::gemm_nuts_chain_bytes(d, n_rows, max_tree_depth); }
extern "C" uint64_t mi_mcmc_test_gemm_nuts_bounded_chain_bytes(uint32_t d, uint32_t n_rows, uint32_t max_tree_depth) { return mi::gemm::gemm_nuts_chain_bytes(d, n_rows, max_tree_depth, true); }
extern "C" uint64_t mi_mcmc_test_gemm_nuts_fixed_bytes(uint32_t d, uint32_t n_rows) { return mi::gemm::gemm_nuts_fixed_bytes(d, n_rows); }
extern "C" uint64_t mi_mcmc_test_gemm_nuts_range_chains(uint64_t n_chains, uint64_t chain_bytes, uint64_t fixed_bytes, uint64_t budget)
{
    return mi::gemm::gemm_nuts_range_chains(n_chains, (size_t)chain_bytes, (size_t)fixed_bytes, (size_t)budget);
}
// test hooks, declared in mi_mcmc_probes.h, for every sampler of the matrix-product route: never capture a graph (run_gemm, run_gemm_nuts), the memory the capacity
// condition of hmc / mala / rwmh sees (gemm_fits), and what it compares with it (gemm_need_bytes: host arithmetic)
namespace {
std::atomic<int> g_gemm_graph_mode{0};
std::atomic<uint64_t> g_gemm_ws_bytes{0};
enum : int { GEMM_PLAIN = 0, GEMM_DENSE_M = 1, GEMM_BOUNDED = 2 };
size_t gemm_need_bytes(uint64_t d, uint64_t n, uint64_t C, int variant, bool replay);
}
extern "C" void mi_mcmc_test_set_gemm_graph(int mode) { g_gemm_graph_mode.store(mode, std::memory_order_relaxed); }
extern "C" void mi_mcmc_test_set_gemm_ws_bytes(uint64_t bytes) { g_gemm_ws_bytes.store(bytes, std::memory_order_relaxed); }
extern "C" uint64_t mi_mcmc_test_gemm_need_bytes(uint32_t d, uint32_t n_rows, uint64_t n_chains, int variant, int replay)
{
    return gemm_need_bytes(d, n_rows, n_chains, variant, replay != 0);
}

namespace {

using namespace mi::host;       // fail, need_device, DevBuf (host_common.hpp); WsLease, ws_get, ws_cached_bytes, ws_release (workspace.hpp)

#ifndef MI_NUTS_MOMENTA_MAX_BYTES
#define MI_NUTS_MOMENTA_MAX_BYTES ((size_t)24 << 30)     // the table of momenta of a nuts run (nuts_memo.hpp): 13.6 GB on BASELINE configs[3]
#endif

// ---- literal replay of the non-finite regime (literal.hpp).  The plain throughput kernels flag the chains whose energies /
// proposal densities went non-finite (nf_flag[c] = 1, nf_flag[C] = 1) and leave their outputs alone; the literal kernel, enqueued
// right behind them on the same stream, replays exactly those chains from their initial values (it returns at once when nothing
// was flagged: one scalar load per workgroup).  Flags and the replay's workspace ride behind the caller's own workspace in the
// per-stream cache.
struct ReplayWs {
    uint32_t* flag = nullptr;     // [C + 1]
    double* tbuf = nullptr;       // t_doubles: the target's matrix transposed (literal.hpp reads matrices column-major: coalesced)
    size_t t_doubles = 0;
    double* work = nullptr;
    size_t stride = 0;            // doubles per workgroup
    unsigned n_wg = 0;
    size_t own_bytes = 0;         // the caller's part, rounded up
    size_t total_bytes = 0;
};
// needs_matrix: the replay reads a d x max(d, n_rows) matrix transposed (DENSE precision, LOGISTIC design matrix, a dense precond_mat);
// the separable ISO / DIAG targets of the "any d" elementwise path read none, and their workspace must not grow as d^2
ReplayWs replay_layout(size_t own_bytes, uint64_t C, uint32_t d, uint32_t n_rows, bool mala_bounded, bool needs_matrix = true)
{
    ReplayWs r;
    r.t_doubles = needs_matrix ? (((size_t)d * std::max<size_t>(d, n_rows) + 31) & ~(size_t)31) : 32;
    r.own_bytes = (own_bytes + 255) & ~(size_t)255;
    r.stride = mi::lit::lit_work_doubles(d, n_rows, mala_bounded);
    r.n_wg = (unsigned)std::min<uint64_t>(C, mala_bounded ? 128u : 512u);
    const size_t flag_bytes = ((C + 1) * sizeof(uint32_t) + 255) & ~(size_t)255;
    r.total_bytes = r.own_bytes + flag_bytes + (r.t_doubles + (size_t)r.n_wg * r.stride) * sizeof(double);
    return r;
}
int replay_bind(ReplayWs& r, void* base, uint64_t C, hipStream_t st)
{
    char* b = static_cast<char*>(base);
    r.flag = reinterpret_cast<uint32_t*>(b + r.own_bytes);
    const size_t flag_bytes = ((C + 1) * sizeof(uint32_t) + 255) & ~(size_t)255;
    r.tbuf = reinterpret_cast<double*>(b + r.own_bytes + flag_bytes);
    r.work = r.tbuf + r.t_doubles;
    HIP_TRY(hipMemsetAsync(r.flag, 0, (C + 1) * sizeof(uint32_t), st));
    return MI_OK;
}
// out[c * rows + r] = in[r * cols + c] on the device (small matrices: the d x d precision, the n x d design matrix)
__global__ void transpose_small_kernel(const double* __restrict__ in, double* __restrict__ out, uint32_t rows, uint32_t cols)
{
    const size_t n = (size_t)rows * cols;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t c = e / rows, r = e % rows;        // consecutive threads write consecutive addresses
        out[e] = in[r * cols + c];
    }
}
int transpose_on_device(const double* in, double* out, uint32_t rows, uint32_t cols, hipStream_t st)
{
    const size_t n = (size_t)rows * cols;
    hipLaunchKernelGGL(transpose_small_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, st, in, out, rows, cols);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// the Gaussian kinds as the literal kernels read them: ISO / DIAG are ELEMENT-WISE targets in the oracle (prec_i * theta_i), DENSE a
// mat-vec.  P_dense: the d*d device matrix of the MFMA path (diagonal for ISO / DIAG), or nullptr with prec_vec (d values / nullptr)
int lit_gauss_target(mi::lit::LitTarget& t, int kind, uint32_t d, const double* P_dense, const double* prec_vec, double* tbuf, hipStream_t st)
{
    t = mi::lit::LitTarget{};
    t.d = d;
    if (kind == MI_TARGET_GAUSS_DENSE) {                 // the literal kernels read the precision transposed
        t.kind = mi::lit::LIT_DENSE; t.prec = tbuf;
        const int rc = transpose_on_device(P_dense, tbuf, d, d, st);
        if (rc) return rc;
    }
    else if (kind == MI_TARGET_GAUSS_DIAG) {
        t.kind = mi::lit::LIT_DIAG;
        if (P_dense) { t.prec = P_dense; t.prec_stride = d + 1; } else { t.prec = prec_vec; t.prec_stride = 1; }
    } else t.kind = mi::lit::LIT_ISO;
    mi::lit::lit_orders(t);
    return MI_OK;
}
void lit_common(mi::lit::LitParams& p, const mi_settings* s, const mi_chains* dev_chains, const ReplayWs& r, bool all_chains)
{
    p.C = dev_chains->n_chains; p.chain0 = dev_chains->chain0;
    p.theta = dev_chains->theta; p.draws = dev_chains->draws; p.n_accept = dev_chains->n_accept; p.n_leap = dev_chains->n_leapfrogs;
    p.seed = s->rng_seed_value;
    p.n_burnin = (uint32_t)s->n_burnin_draws; p.n_keep = (uint32_t)s->n_keep_draws; p.n_leap_steps = (uint32_t)s->n_leap_steps;
    p.draw0 = (uint32_t)dev_chains->draw0; p.eps = s->step_size;
    p.flag = all_chains ? nullptr : r.flag;
    p.any = all_chains ? nullptr : r.flag + p.C;
    p.work = r.work; p.work_stride = r.stride;
}

// One table on the device: n entries of src, padded to n_padded entries with `fill` (settings_host.hpp: pad_table).  The buffer dies with the
// DevBuf, so a caller that uploaded anything synchronises the stream before the DevBuf goes out of scope.
template <class T>
int upload_padded(DevBuf& b, const T* src, size_t n, size_t n_padded, T fill)
{
    std::vector<T> padded;
    if (n_padded > n) { padded.resize(n_padded); mi::settings::pad_table(src, n, n_padded, fill, padded.data()); src = padded.data(); }
    HIP_TRY(b.alloc(n_padded * sizeof(T)));
    HIP_TRY(hipMemcpy(b.p, src, n_padded * sizeof(T), hipMemcpyHostToDevice));
    return MI_OK;
}

// device copies of a LitPrep (literal_host.hpp) and the LitParams pointers into them.  The buffers die with the LitDev, so a caller
// that uploaded anything synchronises the stream before it returns.
struct LitDev {
    DevBuf bt, lb, ub, m, ms, mi, Mfull, Lchol, Minv, sinv_diag, Sinv;
    bool any = false;
};
int lit_upload(const mi::lit::LitPrep& pr, uint32_t d, bool want_bounds, LitDev& dv, mi::lit::LitParams& p)
{
    auto up = [&](DevBuf& b, const std::vector<double>& v, const double*& out) -> int {
        const int rc = upload_padded(b, v.data(), v.size(), v.size(), 0.0);
        dv.any = true; out = b.as<double>();
        return rc;
    };
    int rc;
    p.precond = pr.precond;
    p.rs = pr.rs; p.log_det = pr.log_det; p.cons_term = pr.cons_term;
    if (want_bounds) {
        if ((rc = upload_padded(dv.bt, pr.bt.data(), d, d, 1)) || (rc = up(dv.lb, pr.lb, p.lb)) || (rc = up(dv.ub, pr.ub, p.ub))) return rc;
        p.vals_bound = 1; p.btype = dv.bt.as<int>();
    }
    if (pr.precond == 1) {
        if ((rc = up(dv.m, pr.m, p.m)) || (rc = up(dv.ms, pr.m_sqrt, p.m_sqrt)) || (rc = up(dv.mi, pr.m_inv, p.m_inv))) return rc;
    } else if (pr.precond == 2) {
        if ((rc = up(dv.Mfull, pr.Mfull, p.Mfull)) || (rc = up(dv.Lchol, pr.Lchol, p.Lchol)) || (rc = up(dv.Minv, pr.Minv, p.Minv))) return rc;
    }
    if (!pr.sinv_diag.empty() && (rc = up(dv.sinv_diag, pr.sinv_diag, p.sinv_diag))) return rc;
    if (!pr.Sinv.empty() && (rc = up(dv.Sinv, pr.Sinv, p.Sinv))) return rc;
    return MI_OK;
}

// ---- the literal kernels as the device path of everything the tiled kernels do not implement: dense-gradient targets with d > 128,
// the logistic target with bounds / a preconditioner / nuts beyond d = 8 or with d > 512, max_tree_depth > 10.  One workgroup per
// chain, the reference's operations as written (literal.hpp): O(d^2) per leapfrog step and chain, no MFMA, no shared tiles -- a
// completeness path, not a throughput path.  algo: 0 hmc, 1 mala, 2 nuts, 3 rwmh.
int run_literal(const char* who, int algo, const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st);

// nuts continuation rules (mi_mcmc.h: mi_chains.draw0 / nuts_adapt_state); *n_adapt = the RUN's adaptation window
int nuts_continuation(const mi_settings* s, const mi_chains* c, uint32_t* n_adapt)
{
    *n_adapt = (uint32_t)(s->n_adapt_draws > 0xffffffffULL ? 0xffffffffULL : s->n_adapt_draws);
    if (c->draw0 > 0) {
        if (!c->step_size) return fail(MI_ERR_BAD_ARG, "nuts: a continuation needs chains.step_size (the step sizes of the previous call)");
        if (c->draw0 <= s->n_adapt_draws && !c->nuts_adapt_state)
            return fail(MI_ERR_BAD_ARG, "nuts: a continuation that starts inside or at the end of the adaptation window (draw0 <= n_adapt_draws) needs chains.nuts_adapt_state of the previous call");
    }
    return MI_OK;
}

// Dense d x d precision on the device for the Gaussian kinds (ISO / DIAG expand to a diagonal
// matrix: an fma chain over exact zeros reproduces prec_i * theta_i bit for bit).
int dense_precision_on_device(const mi_target* t, DevBuf& owned, const double** P_dev, hipStream_t st)
{
    const size_t d = t->d;
    if (t->kind == MI_TARGET_GAUSS_DENSE) {
        if (!t->prec) return fail(MI_ERR_BAD_ARG, "GAUSS_DENSE needs prec (d*d)");
        if (t->mem == MI_MEM_DEVICE) { *P_dev = t->prec; return MI_OK; }
        HIP_TRY(owned.alloc(d * d * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(owned.p, t->prec, d * d * sizeof(double), hipMemcpyHostToDevice, st));
        *P_dev = owned.as<double>();
        return MI_OK;
    }
    std::vector<double> diag(d, 1.0);
    if (t->kind == MI_TARGET_GAUSS_DIAG) {
        if (!t->prec) return fail(MI_ERR_BAD_ARG, "GAUSS_DIAG needs prec (d)");
        if (t->mem == MI_MEM_DEVICE) {                   // in the order of the caller's stream: a non-blocking stream that produced prec does not order itself before a NULL-stream copy
            HIP_TRY(hipMemcpyAsync(diag.data(), t->prec, d * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        else
            std::memcpy(diag.data(), t->prec, d * sizeof(double));
    } else if (t->kind != MI_TARGET_GAUSS_ISO) {
        return fail(MI_ERR_UNSUPPORTED, "target kind %d has no dense-precision form", t->kind);
    }
    std::vector<double> P(d * d, 0.0);
    for (size_t i = 0; i < d; ++i) P[i * d + i] = diag[i];
    HIP_TRY(owned.alloc(d * d * sizeof(double)));
    HIP_TRY(hipMemcpy(owned.p, P.data(), d * d * sizeof(double), hipMemcpyHostToDevice));
    *P_dev = owned.as<double>();
    return MI_OK;
}

// n_leapfrogs for the samplers whose kernels do not count leapfrog steps themselves (mala / rwmh: 0; hmc on the logistic
// target: n_total * n_leap_steps), so that the caller's array is defined after every call, host or device memory
__global__ void fill_u64_kernel(uint64_t* out, uint64_t n, uint64_t v)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v;
}

}  // namespace

// ---- what mass_adapt.hip calls too (sampler_host.hpp declares it, with StagedChains)
namespace mi::host {
int check_common(const mi_target* t, const mi_settings* s, const mi_chains* c, bool mass_allowed)
{
    if (!t || !s || !c) return fail(MI_ERR_BAD_ARG, "null target / settings / chains");
    mi::snapshot_grid_cap();
    if (t->struct_size != sizeof(mi_target) || s->struct_size != sizeof(mi_settings) ||
        c->struct_size != sizeof(mi_chains))
        return fail(MI_ERR_BAD_ARG, "struct_size mismatch (header / library version skew)");
    if (c->n_leapfrogs_executed && !c->n_leapfrogs) return fail(MI_ERR_BAD_ARG, "n_leapfrogs_executed needs n_leapfrogs next to it");
    if (t->d == 0 || c->n_chains == 0) return fail(MI_ERR_BAD_ARG, "d and n_chains must be positive");
    if (!c->theta) return fail(MI_ERR_BAD_ARG, "chains.theta is required");
    if (c->mass_diag && !mass_allowed) return fail(MI_ERR_UNSUPPORTED, "chains.mass_diag (per-chain diagonal masses) is implemented for mi_mcmc_hmc_run only");
    if (c->mass_diag && s->precond_mat) return fail(MI_ERR_BAD_ARG, "chains.mass_diag and settings.precond_mat are two mass matrices: one of them must be NULL");
    if (c->draw0 + s->n_burnin_draws + s->n_keep_draws > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "draw0 + draws exceeds the 32-bit draw counter");
    return need_device();
}

// host <-> device staging of one mi_chains shard (StagedChains: sampler_host.hpp)
int stage_in(const mi_chains* c, uint64_t d, uint64_t n_keep, StagedChains& sc, hipStream_t st, uint64_t n_total)
{
    // (every route passes here -- the tile- and user-target entry points do not go through check_common: stage_out copies n_leapfrogs into
    //  n_leapfrogs_executed for every kernel that executes what it counts, so the latter without the former is a bad argument, not a late HIP error)
    if (c->n_leapfrogs_executed && !c->n_leapfrogs) return fail(MI_ERR_BAD_ARG, "n_leapfrogs_executed needs n_leapfrogs next to it");
    mi::snapshot_grid_cap();
    sc.dev = *c;
    if (c->mem == MI_MEM_DEVICE) return MI_OK;
    const size_t C = c->n_chains;
    HIP_TRY(sc.theta.alloc(d * C * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(sc.theta.p, c->theta, d * C * sizeof(double), hipMemcpyHostToDevice, st));
    sc.dev.theta = sc.theta.as<double>();
    if (c->draws) { HIP_TRY(sc.draws.alloc(n_keep * d * C * sizeof(double))); sc.dev.draws = sc.draws.as<double>(); }
    if (c->n_accept) { HIP_TRY(sc.n_accept.alloc(C * sizeof(uint64_t))); sc.dev.n_accept = sc.n_accept.as<uint64_t>(); }
    if (c->step_size) {
        HIP_TRY(sc.step.alloc(C * sizeof(double))); sc.dev.step_size = sc.step.as<double>();
        // in: the adapted step sizes of a nuts continuation; out: written by nuts only -- every other sampler hands the
        // caller's values back unchanged (never uninitialised device memory)
        HIP_TRY(hipMemcpyAsync(sc.step.p, c->step_size, C * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (c->n_leapfrogs) {
        HIP_TRY(sc.n_leap.alloc(C * sizeof(uint64_t))); sc.dev.n_leapfrogs = sc.n_leap.as<uint64_t>();
        HIP_TRY(hipMemsetAsync(sc.n_leap.p, 0, C * sizeof(uint64_t), st));    // samplers without leapfrog steps (mala, rwmh) report 0
    }
    if (c->n_leapfrogs_executed) {
        HIP_TRY(sc.n_exec.alloc(C * sizeof(uint64_t))); sc.dev.n_leapfrogs_executed = sc.n_exec.as<uint64_t>();
        HIP_TRY(hipMemsetAsync(sc.n_exec.p, 0, C * sizeof(uint64_t), st));
    }
    if (c->nuts_depth) { HIP_TRY(sc.depth.alloc(n_total * C * sizeof(uint32_t))); sc.dev.nuts_depth = sc.depth.as<uint32_t>(); }
    if (c->nuts_adapt_state) {                           // in (a continuation inside the adaptation window) / out
        HIP_TRY(sc.adapt.alloc(3 * C * sizeof(double))); sc.dev.nuts_adapt_state = sc.adapt.as<double>();
        HIP_TRY(hipMemcpyAsync(sc.adapt.p, c->nuts_adapt_state, 3 * C * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (c->mass_diag) {
        HIP_TRY(sc.mass.alloc(d * C * sizeof(double))); sc.dev.mass_diag = sc.mass.as<double>();
        HIP_TRY(hipMemcpyAsync(sc.mass.p, c->mass_diag, d * C * sizeof(double), hipMemcpyHostToDevice, st));
    }
    sc.dev.mem = MI_MEM_DEVICE;
    return MI_OK;
}

int stage_out(const mi_chains* c, uint64_t d, uint64_t n_keep, StagedChains& sc, hipStream_t st, uint64_t n_total)
{
    // every kernel but nuts_gauss_memo_kernel executes exactly the leapfrogs it counts
    if (c->n_leapfrogs_executed && !sc.exec_written)
        HIP_TRY(hipMemcpyAsync(sc.dev.n_leapfrogs_executed, sc.dev.n_leapfrogs, c->n_chains * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    if (c->mem == MI_MEM_DEVICE) return MI_OK;
    const size_t C = c->n_chains;
    HIP_TRY(hipMemcpyAsync(c->theta, sc.dev.theta, d * C * sizeof(double), hipMemcpyDeviceToHost, st));
    if (c->draws) HIP_TRY(hipMemcpyAsync(c->draws, sc.dev.draws, n_keep * d * C * sizeof(double), hipMemcpyDeviceToHost, st));
    if (c->n_accept) HIP_TRY(hipMemcpyAsync(c->n_accept, sc.dev.n_accept, C * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (c->step_size) HIP_TRY(hipMemcpyAsync(c->step_size, sc.dev.step_size, C * sizeof(double), hipMemcpyDeviceToHost, st));
    if (c->n_leapfrogs) HIP_TRY(hipMemcpyAsync(c->n_leapfrogs, sc.dev.n_leapfrogs, C * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (c->n_leapfrogs_executed) HIP_TRY(hipMemcpyAsync(c->n_leapfrogs_executed, sc.dev.n_leapfrogs_executed, C * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (c->nuts_depth) HIP_TRY(hipMemcpyAsync(c->nuts_depth, sc.dev.nuts_depth, n_total * C * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (c->nuts_adapt_state) HIP_TRY(hipMemcpyAsync(c->nuts_adapt_state, sc.dev.nuts_adapt_state, 3 * C * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int fill_n_leap(uint64_t* dev_ptr, uint64_t n, uint64_t v, hipStream_t st)
{
    if (!dev_ptr) return MI_OK;
    hipLaunchKernelGGL(fill_u64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dev_ptr, n, v);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
}  // namespace mi::host

namespace {

// identity tables of the general kernel variants (no bounds, unit mass) in stream-ordered workspace memory: what a replay of the
// plain case through a general variant reads (no host buffer has to outlive the call)
// nuts_gauss_memo_kernel: a flagged chain was replayed by the general variant, which executes every leapfrog it counts
__global__ void copy_flagged_counts_kernel(const uint32_t* flag, const uint64_t* n_leap, uint64_t* n_exec, uint64_t C)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C && flag[c] != 0u) n_exec[c] = n_leap[c];
}

__global__ void fill_identity_tables_kernel(int* bt, double* lb, double* ub, double* ms, double* mi, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { bt[i] = 1; lb[i] = 0.0; ub[i] = 0.0; ms[i] = 1.0; mi[i] = 1.0; }
}

int copy_flagged_counts(const uint32_t* flag, const uint64_t* n_leap, uint64_t* n_exec, uint64_t C, hipStream_t st)
{
    hipLaunchKernelGGL(copy_flagged_counts_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, flag, n_leap, n_exec, C);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// ---- what every route states once: the target's data on the device, the launch fields all params structs share, the end of a call
// The matrix of the target in device memory: the n_rows x d design matrix and the labels of MI_TARGET_LOGISTIC (a host target is copied up), the dense
// d x d precision of the Gaussian kinds (dense_precision_on_device; y stays null).  The copy dies with the owner: a route that owns() one synchronises
// the stream before it returns.
struct StagedTarget {
    DevBuf Xo, yo;
    const double *mat = nullptr, *y = nullptr;
    uint64_t n_rows = 0;                                 // (Gaussian kinds: d)
    bool owns() const { return Xo.p != nullptr; }
};
int stage_target(const mi_target* t, StagedTarget& tg, hipStream_t st, uint64_t max_rows = ~0ULL)
{
    const uint64_t d = t->d, n = t->n_rows;
    if (t->kind != MI_TARGET_LOGISTIC) { tg.n_rows = d; return dense_precision_on_device(t, tg.Xo, &tg.mat, st); }
    if (!t->X || !t->y || n == 0 || n > max_rows) return fail(MI_ERR_BAD_ARG, "LOGISTIC needs X, y, n_rows");
    tg.mat = t->X; tg.y = t->y; tg.n_rows = n;
    if (t->mem == MI_MEM_HOST) {
        HIP_TRY(tg.Xo.alloc(n * d * sizeof(double))); HIP_TRY(tg.yo.alloc(n * sizeof(double)));
        HIP_TRY(hipMemcpy(tg.Xo.p, t->X, n * d * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(tg.yo.p, t->y, n * sizeof(double), hipMemcpyHostToDevice));
        tg.mat = tg.Xo.as<double>(); tg.y = tg.yo.as<double>();
    }
    return MI_OK;
}
// ... as the literal replay behind such a route reads it: the matrix transposed into tbuf (literal.hpp reads matrices column-major)
int lit_staged_target(mi::lit::LitTarget& t, const StagedTarget& tg, uint32_t d, double* tbuf, hipStream_t st)
{
    const int rc = transpose_on_device(tg.mat, tbuf, (uint32_t)tg.n_rows, d, st);
    if (rc) return rc;
    t.d = d;
    if (tg.y) { t.kind = mi::lit::LIT_LOGISTIC; t.n_rows = (uint32_t)tg.n_rows; t.X = tg.mat; t.y = tg.y; t.Xt = tbuf; }
    else { t.kind = mi::lit::LIT_DENSE; t.prec = tbuf; }
    mi::lit::lit_orders(t);
    return MI_OK;
}

// the ten fields every params struct has under the same names (what differs in meaning between them -- n_leap, eps / par_scale -- stays with the route)
template <class P>
void fill_common(P& p, uint64_t d, const mi_settings* s, const mi_chains* c, const StagedChains& sc)
{
    p.d = (uint32_t)d; p.C = c->n_chains; p.chain0 = c->chain0;
    p.theta = sc.dev.theta; p.draws = sc.dev.draws; p.n_accept = sc.dev.n_accept;
    p.seed = s->rng_seed_value;
    p.n_burnin = (uint32_t)s->n_burnin_draws; p.n_keep = (uint32_t)s->n_keep_draws;
    p.draw0 = (uint32_t)c->draw0;
}
// nuts: the continuation rules, the depth and the dual-averaging constants ...
template <class P>
int fill_nuts_adapt(P& p, const mi_settings* s, const mi_chains* c)
{
    if (int rc = nuts_continuation(s, c, &p.n_adapt)) return rc;
    p.max_depth = (uint32_t)s->max_tree_depth;
    p.delta = s->target_accept_rate; p.gamma = s->gamma_val; p.t0 = s->t0_val; p.kappa = s->kappa_val;
    return MI_OK;
}
// ... and its three outputs (GemmNutsRun names them differently: it takes the first half alone)
template <class P>
int fill_nuts(P& p, const mi_settings* s, const mi_chains* c, const StagedChains& sc)
{
    p.step_out = sc.dev.step_size; p.depth_trace = sc.dev.nuts_depth; p.adapt_state = sc.dev.nuts_adapt_state;
    return fill_nuts_adapt(p, s, c);
}

// the end of a route: n_leapfrogs of the samplers whose kernels do not count (fill_n_leap; NO_LEAP_FILL: the kernel counted), the outputs back to a host
// caller, and the stream idle before anything of `ours` -- a staged target, tables -- dies with the route
constexpr uint64_t NO_LEAP_FILL = ~0ULL;
int finish(mi_chains* chains, uint64_t d, const mi_settings* s, StagedChains& sc, hipStream_t st, uint64_t leap_fill, bool ours, uint64_t n_total = 0)
{
    int rc;
    if (leap_fill != NO_LEAP_FILL && (rc = fill_n_leap(sc.dev.n_leapfrogs, chains->n_chains, leap_fill, st))) return rc;
    if ((rc = stage_out(chains, d, s->n_keep_draws, sc, st, n_total))) return rc;
    if (ours || chains->mem == MI_MEM_HOST) HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}
uint64_t hmc_leap_total(const mi_settings* s) { return (s->n_burnin_draws + s->n_keep_draws) * s->n_leap_steps; }

// LDS-staged logistic kernels (logistic_lds.hip): workspace from the per-stream cache, launch in their own translation unit
int launched(const char* what, int hip_err);
struct LdsTables;
void lds_tables_replay(const LdsTables& t, const mi::LogitParams& q, mi::lit::LitParams& lp);
bool lds_tables_active(const LdsTables* t);
int launch_logit(int algo, mi::LogitParams prm, const StagedTarget& tg, hipStream_t st,
                 const mi_settings* settings, const mi_chains* dev_chains, int lds_target, const LdsTables* lt)
{
    const double *X_dev = tg.mat, *y_dev = tg.y;
    WsLease base;
    const bool replay = algo != mi::LOGIT_RWMH;          // rwmh forms no product with a vector that can be non-finite (rwmh.cpp:126)
    ReplayWs rp = replay_layout(mi::logit_lds_workspace_bytes(prm.d, prm.NB, prm.C, lds_target), prm.C, prm.d, prm.n_rows, false);
    int rcw = ws_get(st, replay ? rp.total_bytes : rp.own_bytes, base);
    if (rcw) return rcw;
    if (replay) {
        rcw = replay_bind(rp, base.p, prm.C, st);
        if (rcw) return rcw;
        prm.nf_flag = rp.flag;
    }
    // hmc / mala with a DENSE precond_mat (prm.L_rm and the sampler's other matrices from the caller): their block images live in a buffer of their own
    const bool dense_m = prm.L_rm != nullptr;
    DevBuf mws;
    if (dense_m) HIP_TRY(mws.alloc(mi::logit_lds_dense_m_bytes(prm.d, prm.C, lds_target, algo)));
    const int e = dense_m ? mi::logit_lds_launch_dense_m(algo, prm, X_dev, y_dev, base.p, mws.p, st, lds_target)
                          : mi::logit_lds_launch(algo, prm, X_dev, y_dev, base.p, st, lds_target);
    if (e != 0) return fail(MI_ERR_HIP, "LDS-streamed kernel launch: %s", hipGetErrorString((hipError_t)e));
    LitDev ldev;
    if (replay) {                                       // chains that reached the non-finite regime: replayed literally (literal.hpp)
        mi::lit::LitParams lp{};
        rcw = lit_staged_target(lp.t, tg, prm.d, rp.tbuf, st);      // eta = X beta resp. P x read the matrix transposed (literal.hpp)
        if (rcw) return rcw;
        lit_common(lp, settings, dev_chains, rp, false);
        lp.rs = prm.rs; lp.log_det = prm.log_det; lp.cons_term = prm.cons_term;
        if (dense_m) {                                   // the replay's own copies (transposed: literal_host.hpp)
            mi::lit::LitPrep prep;
            rcw = mi::lit::lit_prepare(algo == mi::LOGIT_MALA ? 1 : 0, prm.d, settings->step_size, 0, nullptr, nullptr, settings->precond_mat, prep);
            if (rcw) return rcw;
            rcw = lit_upload(prep, prm.d, false, ldev, lp);      // (mala: INV(Sigma), LOG_DET and the constant term with it)
            if (rcw) return rcw;
        }
        else if (lds_tables_active(lt)) lds_tables_replay(*lt, prm, lp);      // hmc: bounds and / or a diagonal precond_mat
        else if (prm.m_sqrt != nullptr) {                // a diagonal precond_mat (mala: m, m_sqrt, s_inv)
            lp.precond = 1; lp.m = prm.m; lp.m_sqrt = prm.m_sqrt; lp.m_inv = prm.m_inv; lp.sinv_diag = prm.s_inv;
        }
        rcw = launched("LDS-streamed kernel (literal replay)", mi::launch_literal(algo == mi::LOGIT_MALA ? 1 : 0, lp, rp.n_wg, st));
        if (rcw) return rcw;
    }
    if (dense_m) HIP_TRY(hipStreamSynchronize(st));      // the images and the replay's matrices are ours
    return MI_OK;
}

// d x d row-major -> MFMA A-fragment order [t][s][lane] = M[16 t + (lane & 15)][4 s + (lane >> 4)], zero padded to 16 nt
// (what stage_precision writes into LDS): the layout of matrices a kernel reads straight from global memory (d > 64:
// INV / CHOL_LOWER of a dense precond_mat do not fit into LDS next to the precision, hmc_dense.hpp: matvec_mfma_g)
std::vector<double> pack_fragments(const std::vector<double>& M, size_t d, int nt)
{
    const int ns = 4 * nt;
    std::vector<double> out((size_t)nt * ns * 64, 0.0);
    for (int t = 0; t < nt; ++t)
        for (int sl = 0; sl < ns; ++sl)
            for (int l = 0; l < 64; ++l) {
                const size_t row = 16 * (size_t)t + (l & 15), col = 4 * (size_t)sl + (l >> 4);
                if (row < d && col < d) out[((size_t)t * ns + sl) * 64 + l] = M[row * d + col];
            }
    return out;
}
// the device copy of a second / third matrix: row-major for d <= 64 (the kernel stages it into LDS), fragment order beyond
int upload_matrix(const std::vector<double>& M, size_t d, DevBuf& buf)
{
    const int nt = (int)((d + 15) / 16);
    if (nt > 4) {
        const std::vector<double> f = pack_fragments(M, d, 8);
        HIP_TRY(buf.alloc(f.size() * 8));
        HIP_TRY(hipMemcpy(buf.p, f.data(), f.size() * 8, hipMemcpyHostToDevice));
    } else {
        HIP_TRY(buf.alloc(d * d * 8));
        HIP_TRY(hipMemcpy(buf.p, M.data(), d * d * 8, hipMemcpyHostToDevice));
    }
    return MI_OK;
}

// Per-dimension tables of the general kernel variants (settings.vals_bound and / or a diagonal precond_mat):
// determine_bounds_type (determine_bounds_type.hpp:27-57: 1 none, 2 lower, 3 upper, 4 both), the bounds, and the diagonal of
// precond_mat with its CHOL_LOWER / INV (element-wise sqrt / reciprocal for a diagonal matrix, as the oracle's BMO shim gives).
struct GeneralTables {
    bool active = false;
    bool dense = false;                       // precond_mat has off-diagonal entries: INV / CHOL_LOWER as dense matrices
    DevBuf minv_full, l_full;
    std::vector<double> m, m_sqrt, m_inv;     // host copies: the diagonal (of a DENSE matrix too), ones for the identity
    std::vector<double> L;                    // host copy of CHOL_LOWER (dense), row-major
    DevBuf bt, lb, ub, ms_dev, mi_dev;
    DevBuf m_dev;                             // mala alone reads m on the device: upload_m()
    int upload_m() { return upload_padded(m_dev, m.data(), m.size(), m.size(), 1.0); }
};

int general_tables(const char* who, const mi_settings* s, uint64_t d, GeneralTables& g, bool allow_dense = false, bool dense_beyond_64 = false)
{
    namespace S = mi::settings;
    g.active = s->vals_bound != 0 || s->precond_mat != nullptr;
    if (!g.active) return MI_OK;
    if (d > 128) return fail(MI_ERR_UNSUPPORTED, "%s: vals_bound / precond_mat with d > 128 is not implemented", who);
    if (s->vals_bound && (!s->lower_bounds || !s->upper_bounds)) return fail(MI_ERR_BAD_ARG, "%s: vals_bound needs lower_bounds and upper_bounds", who);
    g.m.assign(d, 1.0); g.m_sqrt.assign(d, 1.0); g.m_inv.assign(d, 1.0);
    g.dense = S::precond_kind(s->precond_mat, d) == 2;
    if (g.dense && !allow_dense) return fail(MI_ERR_UNSUPPORTED, "%s: only a diagonal precond_mat is implemented on the device path", who);
    if (s->precond_mat) S::diag_mass(s->precond_mat, d, g.m.data(), g.m_sqrt.data(), g.m_inv.data());
    int rc;
    if (g.dense) {
        if (d > 64 && !dense_beyond_64) return fail(MI_ERR_UNSUPPORTED, "%s: a dense precond_mat / cov_mat is implemented for d <= 64 (diagonal: d <= 128)", who);
        std::vector<double> Minv;
        if ((rc = S::dense_mass(s->precond_mat, d, &Minv, g.L)) || (rc = upload_matrix(Minv, d, g.minv_full)) || (rc = upload_matrix(g.L, d, g.l_full))) return rc;
    }
    std::vector<int> bt(d);
    std::vector<double> lbv(d), ubv(d);
    S::bounds_tables(d, s->vals_bound ? 1 : 0, s->lower_bounds, s->upper_bounds, bt.data(), lbv.data(), ubv.data());
    if ((rc = upload_padded(g.bt, bt.data(), d, d, 1)) || (rc = upload_padded(g.lb, lbv.data(), d, d, 0.0)) || (rc = upload_padded(g.ub, ubv.data(), d, d, 0.0))
        || (rc = upload_padded(g.ms_dev, g.m_sqrt.data(), d, d, 1.0)) || (rc = upload_padded(g.mi_dev, g.m_inv.data(), d, d, 1.0))) return rc;
    return MI_OK;
}

// Kernel families live in their own translation units (launchers.hpp); these wrappers turn their hipError_t into a status.
int launched(const char* what, int hip_err)
{
    if (hip_err != 0) return fail(MI_ERR_HIP, "%s kernel launch: %s", what, hipGetErrorString((hipError_t)hip_err));
    return MI_OK;
}

// per-chain diagonal masses (mi_chains.mass_diag, [d][C]): CHOL_LOWER and INV of a diagonal matrix are the element-wise sqrt(m) and
// 1 / m (what the oracle's Cholesky / Gauss-Jordan give for diag(m)), formed on the device next to the masses
__global__ void chain_mass_tables_kernel(const double* __restrict__ mass, uint64_t n, double* __restrict__ m_sqrt, double* __restrict__ m_inv)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) { const double m = mass[e]; m_sqrt[e] = __builtin_sqrt(m); m_inv[e] = 1.0 / m; }
}
struct ChainMass { DevBuf ms, mi; };
int chain_mass_tables(const double* mass_dev, uint64_t d, uint64_t C, ChainMass& t, hipStream_t st)
{
    const uint64_t n = d * C;
    HIP_TRY(t.ms.alloc(n * 8)); HIP_TRY(t.mi.alloc(n * 8));
    hipLaunchKernelGGL(chain_mass_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mass_dev, n, t.ms.as<double>(), t.mi.as<double>());
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
void lit_set_chain_mass(mi::lit::LitParams& lp, const double* mass_dev, const ChainMass& t, uint64_t C)
{
    lp.precond = 1; lp.m = mass_dev; lp.m_sqrt = t.ms.as<double>(); lp.m_inv = t.mi.as<double>(); lp.m_chain_stride = C;
}
// the diagonal masses of a plain launch: per chain (mi_chains.mass_diag, [d][C]) or shared (sqrt(m) and 1 / m of a diagonal precond_mat alone, no bounds), or none
struct HmcMass { ChainMass t; bool per_chain = false, shared = false; };
template <class P>
int hmc_mass(HmcMass& hm, P& q, const mi_settings* settings, const StagedChains& sc, bool shared, hipStream_t st)
{
    int rc;
    const uint64_t d = q.d;
    if (sc.dev.mass_diag) {                              // per-chain tables [d][C]
        if ((rc = chain_mass_tables(sc.dev.mass_diag, d, q.C, hm.t, st))) return rc;
        hm.per_chain = true; q.m_per_chain = 1;
    } else if (shared) {
        std::vector<double> m(d), m_sqrt(d), m_inv(d);
        mi::settings::diag_mass(settings->precond_mat, d, m.data(), m_sqrt.data(), m_inv.data());
        if ((rc = upload_padded(hm.t.ms, m_sqrt.data(), d, d, 1.0)) || (rc = upload_padded(hm.t.mi, m_inv.data(), d, d, 1.0))) return rc;
        hm.shared = true;
    } else return MI_OK;
    q.m_sqrt = hm.t.ms.as<double>(); q.m_inv = hm.t.mi.as<double>();
    return MI_OK;
}

// the target of a literal kernel (literal.hpp: LitTarget) in device memory: a host-memory target is staged into a / b, a matrix the literal
// kernels read transposed into t_t.  The buffers must outlive the launch.
// value_only: the caller never asks for a gradient, so the value-only kinds (MI_TARGET_GAUSS_MIXTURE) are served too.
int lit_stage_target(const char* who, const mi_target* target, mi::lit::LitTarget& t, DevBuf& t_a, DevBuf& t_b, DevBuf& t_t, hipStream_t st,
                     bool value_only = false)
{
    const uint64_t d = target->d;
    t.d = (uint32_t)d;
    auto up = [&](DevBuf& b, const double* src, size_t n_doubles, const double** out) -> int {
        if (target->mem == MI_MEM_DEVICE) { *out = src; return MI_OK; }
        HIP_TRY(b.alloc(n_doubles * 8));
        HIP_TRY(hipMemcpy(b.p, src, n_doubles * 8, hipMemcpyHostToDevice));
        *out = b.as<double>();
        return MI_OK;
    };
    int rc;
    switch (target->kind) {
    case MI_TARGET_GAUSS_ISO: t.kind = mi::lit::LIT_ISO; break;
    case MI_TARGET_GAUSS_DIAG:
        if (!target->prec) return fail(MI_ERR_BAD_ARG, "GAUSS_DIAG needs prec (d)");
        t.kind = mi::lit::LIT_DIAG; t.prec_stride = 1;
        if ((rc = up(t_a, target->prec, d, &t.prec))) return rc;
        break;
    case MI_TARGET_GAUSS_DENSE:
        if (!target->prec) return fail(MI_ERR_BAD_ARG, "GAUSS_DENSE needs prec (d*d)");
        t.kind = mi::lit::LIT_DENSE;
        if ((rc = up(t_a, target->prec, d * d, &t.prec))) return rc;
        HIP_TRY(t_t.alloc(d * d * 8));                     // ... read transposed by the literal kernels
        if ((rc = transpose_on_device(t.prec, t_t.as<double>(), (uint32_t)d, (uint32_t)d, st))) return rc;
        t.prec = t_t.as<double>();
        break;
    case MI_TARGET_LOGISTIC:
        if (!target->X || !target->y || target->n_rows == 0) return fail(MI_ERR_BAD_ARG, "LOGISTIC needs X, y, n_rows");
        t.kind = mi::lit::LIT_LOGISTIC; t.n_rows = (uint32_t)target->n_rows;
        if ((rc = up(t_a, target->X, target->n_rows * d, &t.X))) return rc;
        if ((rc = up(t_b, target->y, target->n_rows, &t.y))) return rc;
        HIP_TRY(t_t.alloc(target->n_rows * d * 8));
        if ((rc = transpose_on_device(t.X, t_t.as<double>(), (uint32_t)target->n_rows, (uint32_t)d, st))) return rc;
        t.Xt = t_t.as<double>();
        break;
    case MI_TARGET_GAUSS_MIXTURE:
        if (!value_only) return fail(MI_ERR_UNSUPPORTED, "%s: MI_TARGET_GAUSS_MIXTURE is value-only (mcmc::aees alone)", who);
        if (!target->X || !target->prec || !target->y || target->n_rows == 0 || target->n_rows > 0xffffffffULL)
            return fail(MI_ERR_BAD_ARG, "GAUSS_MIXTURE needs X (M*d means), prec (M variances), y (M log constants), n_rows = M");
        t.kind = mi::lit::LIT_MIXTURE; t.n_rows = (uint32_t)target->n_rows;
        if ((rc = up(t_a, target->X, target->n_rows * d, &t.X))) return rc;
        if ((rc = up(t_b, target->prec, target->n_rows, &t.prec))) return rc;
        if ((rc = up(t_t, target->y, target->n_rows, &t.y))) return rc;
        break;
    default: return fail(MI_ERR_UNSUPPORTED, "%s: target kind %d not implemented", who, target->kind);
    }
    mi::lit::lit_orders(t);
    return MI_OK;
}

int run_literal(const char* who, int algo, const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st)
{
    const uint64_t d = target->d, C = chains->n_chains;
    const uint64_t n_total = settings->n_burnin_draws + settings->n_keep_draws;
    if (n_total > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "too many draws");
    if (d > 0x7fffffffULL) return fail(MI_ERR_BAD_ARG, "%s: d out of range", who);
    if (settings->vals_bound && (!settings->lower_bounds || !settings->upper_bounds)) return fail(MI_ERR_BAD_ARG, "%s: vals_bound needs lower_bounds and upper_bounds", who);
    if (algo == 2 && settings->max_tree_depth > (uint64_t)mi::lit::LIT_NUTS_MAX_DEPTH)
        return fail(MI_ERR_UNSUPPORTED, "nuts: max_tree_depth > %d not implemented (2^%d leapfrog steps per draw)", (int)mi::lit::LIT_NUTS_MAX_DEPTH, (int)mi::lit::LIT_NUTS_MAX_DEPTH);
    mi::lit::LitParams lp{};
    DevBuf t_a, t_b, t_t;                                // staged target (and its transposed matrix)
    int rc = lit_stage_target(who, target, lp.t, t_a, t_b, t_t, st);
    if (rc) return rc;
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st, n_total);
    if (rc) return rc;
    if (algo == 4 && d > (uint64_t)mi::lit::LIT_RMHMC_MAX_D)
        return fail(MI_ERR_UNSUPPORTED, "rmhmc: d = %llu > %d is not implemented (two d x d x d derivative cubes per chain; O(d^4) per fixed-point step)",
                    (unsigned long long)d, (int)mi::lit::LIT_RMHMC_MAX_D);
    const bool mala_bounded = algo == 1 && settings->vals_bound != 0;
    if (mala_bounded && d > 512) return fail(MI_ERR_UNSUPPORTED, "mala: vals_bound with d > 512 is not implemented (ten d x d matrices per workgroup)");
    ReplayWs rp;
    rp.stride = mi::lit::lit_work_doubles((uint32_t)d, lp.t.n_rows, mala_bounded, (uint32_t)settings->max_tree_depth, algo == 2, algo == 4);
    rp.n_wg = (unsigned)std::min<uint64_t>(C, (mala_bounded || algo == 4) ? 128u : 1024u);
    WsLease ws;
    rc = ws_get(st, (size_t)rp.n_wg * rp.stride * sizeof(double), ws);
    if (rc) return rc;
    rp.work = ws.as<double>();
    lit_common(lp, settings, &sc.dev, rp, true);
    mi::lit::LitPrep prep;
    rc = mi::lit::lit_prepare(algo == 1 ? 1 : 0, (uint32_t)d, settings->step_size, settings->vals_bound ? 1 : 0, settings->lower_bounds,
                              settings->upper_bounds, algo == 4 ? nullptr : settings->precond_mat, prep);     // (rmhmc has no precond_mat)
    if (rc) return rc;
    lp.n_fp_steps = (uint32_t)settings->n_fp_steps;
    LitDev ldev;
    rc = lit_upload(prep, (uint32_t)d, settings->vals_bound != 0, ldev, lp);
    if (rc) return rc;
    ChainMass cm;
    if (sc.dev.mass_diag) {                              // hmc with per-chain diagonal masses (checked by the caller)
        if ((rc = chain_mass_tables(sc.dev.mass_diag, d, C, cm, st))) return rc;
        lit_set_chain_mass(lp, sc.dev.mass_diag, cm, C);
    }
    if (algo == 2 && (rc = fill_nuts(lp, settings, chains, sc))) return rc;
    rc = launched(who, mi::launch_literal(algo, lp, rp.n_wg, st));
    if (rc) return rc;
    return finish(chains, d, settings, sc, st, NO_LEAP_FILL, t_a.p || t_b.p || t_t.p || ldev.any || cm.ms.p, n_total);
}


// ---- mcmc::rmhmc with HOST callbacks (ref: include/mcmc/rmhmc.hpp: target_log_kernel and tensor_fn as std::function): one chain on
// literal_kernel<4> with the LIT_CALLBACK target -- the kernel asks for every evaluation through a mailbox in pinned memory
// (literal.hpp: LitMailbox), this thread serves the requests while the kernel runs.  Everything that is the sampler's own arithmetic
// (fixed-point iterations, INV / CHOL_LOWER / LOG_DET of the metric, the d matrix products of mntm_update_fn, energies, the Metropolis
// test) is on the device; what runs on the host is the user's code, as in the reference.
namespace {
struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes) { return hipHostMalloc(&p, bytes ? bytes : 8, hipHostMallocCoherent); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
// serve the kernel's requests until the stream is idle; returns the number of requests served
uint64_t serve_callbacks(const mi::lit::LitMailbox& mb, uint32_t d, mi_log_kernel_cb kcb, void* kdata, mi_tensor_cb tcb, void* tdata, hipStream_t st)
{
    uint32_t served = 0;
    uint64_t n = 0;
    unsigned idle = 0;
    for (;;) {
        const uint32_t req = __atomic_load_n(&mb.ctl[mi::lit::LIT_MB_REQ], __ATOMIC_ACQUIRE);
        if (req != served) {
            const bool want = mb.ctl[mi::lit::LIT_MB_WANT] != 0u;
            if (mb.ctl[mi::lit::LIT_MB_KIND] == (uint32_t)mi::lit::LIT_REQ_KERNEL) *mb.value = kcb(mb.x, want ? mb.out : nullptr, kdata);
            else tcb(mb.x, mb.out, want ? mb.out + (size_t)d * d : nullptr, tdata);
            __atomic_store_n(&mb.ctl[mi::lit::LIT_MB_ACK], req, __ATOMIC_RELEASE);
            served = req; ++n; idle = 0;
            continue;
        }
        if ((++idle & 0xffu) == 0u) {
            if (hipStreamQuery(st) != hipErrorNotReady) {                            // the kernel has ended (or failed): one last look, then out
                if (__atomic_load_n(&mb.ctl[mi::lit::LIT_MB_REQ], __ATOMIC_ACQUIRE) == served) break;
            }
            std::this_thread::yield();                                              // (between requests the kernel computes: let the core go now and then)
        }
    }
    return n;
}
}  // namespace

// mala with a diagonal precond_mat on the LDS-streamed kernels: m, sqrt(m), INV(eps^2 M) (padded with ones to 512 entries) and LOG_DET(eps^2 M)
// (settings_host.hpp)
struct MalaDiagMass { DevBuf m, ms, sinv; };
int mala_diag_tables(const mi_settings* settings, uint64_t d, MalaDiagMass& t, mi::LogitParams& q)
{
    std::vector<double> m(d), ms(d), mi_(d);
    mi::settings::diag_mass(settings->precond_mat, d, m.data(), ms.data(), mi_.data());
    mi::settings::MalaSigma sg;
    int rc = mi::settings::mala_sigma(d, settings->step_size, 1, m.data(), sg);
    if (rc) return rc;
    if ((rc = upload_padded(t.m, m.data(), d, 512, 1.0)) || (rc = upload_padded(t.ms, ms.data(), d, 512, 1.0))
        || (rc = upload_padded(t.sinv, sg.sinv_diag.data(), d, 512, 1.0))) return rc;
    q.m = t.m.as<double>(); q.m_sqrt = t.ms.as<double>(); q.s_inv = t.sinv.as<double>();
    q.log_det = sg.log_det;
    return MI_OK;
}
bool precond_is_diagonal(const mi_settings* settings, uint64_t d) { return mi::settings::precond_kind(settings->precond_mat, d) == 1; }

// settings.vals_bound and / or a DIAGONAL precond_mat for hmc / nuts on the LDS-streamed kernels (lds_box.hpp; logistic_lds.hpp DIAGM / BOUNDS):
// determine_bounds_type (determine_bounds_type.hpp:27-57), the bounds, sqrt(m) and 1 / m -- on the device, padded to 512 entries with type 1 /
// ones; with bounds the mass tables are always there (ones for the identity)
struct LdsTables { DevBuf bt, lb, ub, m, ms, mi; bool bounds = false, mass = false; };
int lds_tables(const char* who, const mi_settings* settings, uint64_t d, LdsTables& t, mi::LogitParams& q)
{
    t.bounds = settings->vals_bound != 0; t.mass = settings->precond_mat != nullptr;
    if (!t.bounds && !t.mass) return MI_OK;
    if (t.bounds && (!settings->lower_bounds || !settings->upper_bounds)) return fail(MI_ERR_BAD_ARG, "%s: vals_bound needs lower_bounds and upper_bounds", who);
    std::vector<double> m(d, 1.0), ms(d, 1.0), mi_(d, 1.0);
    if (t.mass) mi::settings::diag_mass(settings->precond_mat, d, m.data(), ms.data(), mi_.data());
    int rc;
    if ((rc = upload_padded(t.m, m.data(), d, 512, 1.0)) || (rc = upload_padded(t.ms, ms.data(), d, 512, 1.0)) || (rc = upload_padded(t.mi, mi_.data(), d, 512, 1.0))) return rc;
    q.m_sqrt = t.ms.as<double>(); q.m_inv = t.mi.as<double>();
    if (t.bounds) {
        std::vector<int> bt(d);
        std::vector<double> lbv(d), ubv(d);
        mi::settings::bounds_tables(d, 1, settings->lower_bounds, settings->upper_bounds, bt.data(), lbv.data(), ubv.data());
        if ((rc = upload_padded(t.bt, bt.data(), d, 512, 1)) || (rc = upload_padded(t.lb, lbv.data(), d, 512, 0.0)) || (rc = upload_padded(t.ub, ubv.data(), d, 512, 0.0))) return rc;
        q.btype = t.bt.as<int>(); q.lb = t.lb.as<double>(); q.ub = t.ub.as<double>();
    }
    return MI_OK;
}
// hmc with a DENSE precond_mat on the LDS-streamed kernel (logistic_lds.hpp: DENSEM): INV(M) and CHOL_LOWER(M) from the host (hmc.cpp:57-59
// through the oracle's Gauss-Jordan / column Cholesky, as everywhere), row-major on the device
// mala (mala.cpp:57-58; mala.ipp:58-64): M, CHOL_LOWER(M), and -- Sigma = eps^2 M is constant without bounds -- INV(Sigma) and LOG_DET(Sigma)
// (settings_host.hpp: mala_sigma), as the d <= 128 kernel takes them (mala_gauss_dense_m_kernel)
struct LdsDenseM { DevBuf minv, l, m, sinv; };
int lds_dense_m(const mi_settings* settings, uint64_t d, LdsDenseM& t, mi::LogitParams& q, int algo)
{
    const size_t dd = (size_t)d * d;
    int rc;
    const bool mala = algo == mi::LOGIT_MALA;
    std::vector<double> Minv, L;
    if ((rc = mi::settings::dense_mass(settings->precond_mat, d, mala ? nullptr : &Minv, L)) || (rc = upload_padded(t.l, L.data(), dd, dd, 0.0))) return rc;
    q.L_rm = t.l.as<double>();
    if (mala) {
        mi::settings::MalaSigma sg;
        if ((rc = mi::settings::mala_sigma(d, settings->step_size, 2, settings->precond_mat, sg))) return rc;
        q.log_det = sg.log_det;
        if ((rc = upload_padded(t.m, settings->precond_mat, dd, dd, 0.0)) || (rc = upload_padded(t.sinv, sg.Sinv.data(), dd, dd, 0.0))) return rc;
        q.M_rm = t.m.as<double>(); q.Sinv_rm = t.sinv.as<double>();
    } else {
        if ((rc = upload_padded(t.minv, Minv.data(), dd, dd, 0.0))) return rc;
        q.Minv_rm = t.minv.as<double>();
    }
    return MI_OK;
}
// ... which the hmc and mala front ends route there when this holds (bounds with a dense matrix stay on literal.hpp)
bool lds_dense_m_ok(const mi_target* target, const mi_settings* settings)
{
    return target->kernel_hint != MI_KERNEL_LITERAL && settings->precond_mat && !settings->vals_bound && !precond_is_diagonal(settings, target->d);
}
// the same tables for the literal replay behind such a launch (precond 1: M, sqrt(M), 1 / M element by element; literal_host.hpp)
void lds_tables_replay(const LdsTables& t, const mi::LogitParams& q, mi::lit::LitParams& lp)
{
    if (t.mass) { lp.precond = 1; lp.m = t.m.as<double>(); lp.m_sqrt = q.m_sqrt; lp.m_inv = q.m_inv; }
    if (t.bounds) { lp.vals_bound = 1; lp.btype = q.btype; lp.lb = q.lb; lp.ub = q.ub; }
}
bool lds_tables_active(const LdsTables* t) { return t != nullptr && (t->bounds || t->mass); }
// hmc / nuts cases of settings the LDS-streamed kernels cover: no bounds / bounds, identity / diagonal precond_mat
bool lds_general_ok(const mi_target* target, const mi_settings* settings)
{
    return target->kernel_hint != MI_KERNEL_LITERAL && (!settings->precond_mat || precond_is_diagonal(settings, target->d));
}

// hmc / mala / rwmh on the LDS-streamed kernels (logistic_lds.hpp), 8 < d <= 512: the logistic-regression target (LOGIT_TARGET_LOGISTIC: its design matrix
// is streamed through LDS block by block), and a dense Gaussian with 128 < d (LOGIT_TARGET_DENSE: P no longer fits into LDS, hmc_dense.hpp, so it takes the
// design matrix's place).  Identity, diagonal or -- without bounds -- dense precond_mat (hmc, mala); bounds (hmc); rwmh plain.  settings->step_size is the
// leapfrog step resp. par_scale.
int run_lds(const char* who, int algo, const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st, int lds_target)
{
    int rc;
    const uint64_t d = target->d;
    StagedTarget tg;
    if ((rc = stage_target(target, tg, st))) return rc;
    if (lds_target == mi::LOGIT_TARGET_LOGISTIC && d > 512) return fail(MI_ERR_UNSUPPORTED, "%s: logistic target with d = %llu > 512 not implemented", who, (unsigned long long)d);
    if (settings->n_burnin_draws + settings->n_keep_draws > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "too many draws");
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st);
    if (rc) return rc;
    mi::LogitParams q{};
    fill_common(q, d, settings, chains, sc);
    q.n_rows = (uint32_t)tg.n_rows; q.NB = (uint32_t)((tg.n_rows + 15) / 16);
    q.n_leap = (uint32_t)settings->n_leap_steps;
    q.eps = settings->step_size;
    if (algo == mi::LOGIT_MALA) {                        // dmvnorm's constants for Sigma = eps^2 I, as the oracle states them
        mi::settings::MalaSigma sg;
        (void)mi::settings::mala_sigma(d, settings->step_size, 0, nullptr, sg);
        q.s2 = settings->step_size * settings->step_size; q.rs = sg.rs; q.log_det = sg.log_det; q.cons_term = sg.cons_term;
    }
    LdsTables lt;
    LdsDenseM ldm;
    MalaDiagMass mdm;
    if ((algo == mi::LOGIT_HMC || algo == mi::LOGIT_MALA) && lds_dense_m_ok(target, settings)) { if ((rc = lds_dense_m(settings, d, ldm, q, algo))) return rc; }      // a dense precond_mat, unbounded
    else if (algo == mi::LOGIT_HMC) { if ((rc = lds_tables(who, settings, d, lt, q))) return rc; }      // (the caller routed bounds / a DIAGONAL matrix here)
    else if (algo == mi::LOGIT_MALA && settings->precond_mat) { if ((rc = mala_diag_tables(settings, d, mdm, q))) return rc; }
    rc = launch_logit(algo, q, tg, st, settings, &sc.dev, lds_target, &lt);
    if (rc) return rc;
    return finish(chains, d, settings, sc, st, algo == mi::LOGIT_HMC ? hmc_leap_total(settings) : 0, tg.owns() || lt.ms.p || mdm.m.p);
}

// hmc / mala / rwmh on a dense Gaussian or the logistic-regression target BEYOND d = 512 (identity preconditioner / cov_mat; hmc and rwmh also with bounds): the state of a
// 16-chain tile no longer fits a workgroup, so it lives in HBM and the gradients of ALL chains at one leapfrog step are fp64 matrix products on the matrix
// cores -- W = P Theta, resp. eta = X Theta and X^T (y - sigmoid(eta)) -- with the half-kicks and the drift in the epilogue (gemm_samplers.hip); chains that
// reach the non-finite regime are flagged and replayed by literal.hpp right behind it.  algo: the C ABI's numbers (0 hmc, 1 mala, 3 rwmh).
// A DENSE precond_mat (hmc, mala) rides the same route -- products with INV(M), CHOL_LOWER(M), M, INV(eps^2 M) next to the gradient's -- where the route can hold it:
// what it cannot (a matrix beyond the device factorisations of linalg_device.hip, a launch grid out of range, a workspace -- three more packed matrices, four more
// state vectors -- beyond the free device memory) stays on the literal kernel, as before
constexpr uint64_t GEMM_DENSE_M_MAX_D = LINALG_STAGE_BYTES / (2 * sizeof(double));      // 3840: device_inverse's LDS-staged pivot row
// what the capacity condition compares with the memory there is: the route's workspace (with `replay` the flags and the literal replay's matrix and work areas behind
// it: hmc, mala) and the uploads next to it -- the tables and a host target's matrix; with a dense precond_mat the replay's transposed matrices (lit_upload)
size_t gemm_need_bytes(uint64_t d, uint64_t n, uint64_t C, int variant, bool replay)
{
    const bool dm = variant == GEMM_DENSE_M;
    const ReplayWs rp = replay_layout(mi::gemm::gemm_ws_bytes((uint32_t)d, (uint32_t)n, C, dm, variant == GEMM_BOUNDED), C, (uint32_t)d, (uint32_t)(n ? n : d), false);
    const size_t uploads = (dm ? 4 : 1) * (size_t)d * d * sizeof(double) + ((size_t)1 << 20);
    return ((replay || dm) ? rp.total_bytes : rp.own_bytes) + uploads;
}
// Capacity is a routing condition for every variant: what the route cannot hold (a launch grid out of range; a workspace beyond the free device memory; with a dense
// precond_mat a matrix beyond the device factorisations of linalg_device.hip) stays on the literal kernel, with the same bits.  vals_bound rides the route for hmc
// (identity / DIAGONAL precond_mat) and rwmh (no cov_mat): three more state vectors hold x = inv_transform(theta), what the products read
bool gemm_fits(const mi_target* target, const mi_chains* chains, int variant, bool replay, hipStream_t st)
{
    const uint64_t d = target->d, C = chains->n_chains, n = target->kind == MI_TARGET_LOGISTIC ? target->n_rows : 0;
    if (n > 0x7fffffffULL || (C + 127) / 128 * 2 > 65535) return false;      // (grid.x of the class-wise kernels: Cp / 64)
    if (variant == GEMM_DENSE_M && (d > GEMM_DENSE_M_MAX_D || !linalg_on_device(0, (size_t)d))) return false;
    size_t have = (size_t)g_gemm_ws_bytes.load(std::memory_order_relaxed);      // (the test hook: as if this were all there is)
    if (have == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
        have = free_b + ws_cached_bytes(st);                 // (the cached workspace of this stream is given back before a larger one is taken)
    }
    return gemm_need_bytes(d, n, C, variant, replay) <= have;
}
bool gemm_case(const mi_target* target, const mi_settings* settings, const mi_chains* chains, bool hmc, bool algo_has_mass = true, hipStream_t st = nullptr)
{
    if (!((target->kind == MI_TARGET_GAUSS_DENSE || target->kind == MI_TARGET_LOGISTIC) && target->d > 512
          && !chains->mass_diag && target->kernel_hint != MI_KERNEL_LITERAL && (!hmc || settings->n_leap_steps >= 1))) return false;
    if (target->d > 131056ULL) return false;             // (grid.y of the normals kernel: padded d / 2; gemm_nuts_case has the same guard)
    if (settings->vals_bound) {                          // hmc (identity / diagonal precond_mat) and rwmh (no cov_mat); bounded mala (its proposal covariance is J M per chain) stays literal
        if (!hmc && algo_has_mass) return false;
        if (settings->precond_mat && (!algo_has_mass || !precond_is_diagonal(settings, target->d))) return false;
        if (!settings->lower_bounds || !settings->upper_bounds) return true;      // (run_gemm reports the missing arrays)
        return gemm_fits(target, chains, GEMM_BOUNDED, hmc, st);
    }
    if (settings->precond_mat && !algo_has_mass) return false;                   // rwmh with a cov_mat: the literal kernel
    const bool dense_m = settings->precond_mat && !precond_is_diagonal(settings, target->d);
    return gemm_fits(target, chains, dense_m ? GEMM_DENSE_M : GEMM_PLAIN, algo_has_mass, st);      // (rwmh has no replay: run_gemm)
}
// the mass tables of the matrix-product route: n_tables tables of dK entries in one buffer -- m | sqrt(m) | 1 / m of a diagonal precond_mat, padded with
// ones; everything else (the identity, a dense matrix, a fourth table) ones
void gemm_mass_tables(const mi::lit::LitPrep& prep, uint64_t d, uint32_t dK, int n_tables, std::vector<double>& tabs)
{
    tabs.assign((size_t)n_tables * dK, 1.0);
    if (prep.precond != 1) return;
    mi::settings::pad_table(prep.m.data(), d, dK, 1.0, &tabs[0]);
    mi::settings::pad_table(prep.m_sqrt.data(), d, dK, 1.0, &tabs[dK]);
    mi::settings::pad_table(prep.m_inv.data(), d, dK, 1.0, &tabs[2 * (size_t)dK]);
}
// vals_bound on the matrix-product route (run_gemm, run_gemm_nuts): bounds type, lower and upper bound per dimension (determine_bounds_type.hpp:27-57, from lit_prepare)
// padded with type 1, and per 16-dimension block whether it holds a bounded dimension at all -- the others skip every exp / log
struct GemmBoxTables {
    DevBuf dev;
    const int* btype = nullptr;
    const double *lb = nullptr, *ub = nullptr;
    const uint32_t* blocks = nullptr;
};
int gemm_box_tables(const mi::lit::LitPrep& prep, uint64_t d, uint32_t dK, GemmBoxTables& t)
{
    const size_t off_lb = (size_t)dK * sizeof(int), off_ub = off_lb + (size_t)dK * 8, off_blk = off_ub + (size_t)dK * 8, bytes = off_blk + (size_t)(dK / 16) * sizeof(uint32_t);
    std::vector<unsigned char> host(bytes, 0);
    mi::settings::pad_table(prep.bt.data(), d, dK, 1, reinterpret_cast<int*>(host.data()));
    mi::settings::pad_table(prep.lb.data(), d, dK, 0.0, reinterpret_cast<double*>(host.data() + off_lb));
    mi::settings::pad_table(prep.ub.data(), d, dK, 0.0, reinterpret_cast<double*>(host.data() + off_ub));
    uint32_t* blk = reinterpret_cast<uint32_t*>(host.data() + off_blk);
    for (uint64_t i = 0; i < d; ++i) if (prep.bt[i] != 1) blk[i / 16] = 1u;
    if (int rc = upload_padded(t.dev, host.data(), bytes, bytes, (unsigned char)0)) return rc;
    unsigned char* base = static_cast<unsigned char*>(t.dev.p);
    t.btype = reinterpret_cast<const int*>(base); t.lb = reinterpret_cast<const double*>(base + off_lb);
    t.ub = reinterpret_cast<const double*>(base + off_ub); t.blocks = reinterpret_cast<const uint32_t*>(base + off_blk);
    return 0;
}
int run_gemm(const char* who, int algo, const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st)
{
    int rc;
    const uint64_t d = target->d, C = chains->n_chains;
    const bool logit = target->kind == MI_TARGET_LOGISTIC;
    const uint64_t n = logit ? target->n_rows : 0;
    if (d > 0x7fffffffULL || n > 0x7fffffffULL) return fail(MI_ERR_BAD_ARG, "%s: d / n_rows out of range", who);
    if (settings->n_burnin_draws + settings->n_keep_draws > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "too many draws");
    if (algo == 0 && settings->n_leap_steps > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "hmc: too many leapfrog steps");
    const bool bounded = settings->vals_bound != 0;
    if (bounded && (!settings->lower_bounds || !settings->upper_bounds)) return fail(MI_ERR_BAD_ARG, "%s: vals_bound needs lower_bounds and upper_bounds", who);
    StagedTarget tg;
    if ((rc = stage_target(target, tg, st))) return rc;
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st);
    if (rc) return rc;
    mi::gemm::GemmRun g;
    fill_common(g, d, settings, chains, sc);
    g.algo = algo; g.n_rows = (uint32_t)n;
    if (logit) { g.X = tg.mat; g.y = tg.y; } else g.P = tg.mat;
    g.n_leap = (uint32_t)settings->n_leap_steps; g.eps = settings->step_size;
    // identity or a DIAGONAL precond_mat (hmc.cpp:57-59, mala.cpp:57-58 with mala.ipp:58-64): diag(M), CHOL_LOWER (sqrt), INV (reciprocal) and, mala, INV(eps^2 M) with
    // LOG_DET(eps^2 M) -- all from lit_prepare, in the oracle's operation order; the identity as tables of ones (1.0 * x is x bit for bit)
    mi::lit::LitPrep prep;
    rc = mi::lit::lit_prepare(algo == 1 ? 1 : 0, (uint32_t)d, settings->step_size, bounded ? 1 : 0, settings->lower_bounds, settings->upper_bounds, settings->precond_mat, prep);
    if (rc) return rc;
    const uint32_t dK = mi::gemm::gemm_padded_d((uint32_t)d);
    GemmBoxTables box;
    if (bounded) {
        if ((rc = gemm_box_tables(prep, d, dK, box))) return rc;
        g.bounded = true; g.btype = box.btype; g.lb = box.lb; g.ub = box.ub; g.box_blocks = box.blocks;
    }
    std::vector<double> tabs;
    gemm_mass_tables(prep, d, dK, 4, tabs);
    if (algo == 1) {                                     // dmvnorm's constants for Sigma = eps^2 M, as the oracle states them
        g.s2 = settings->step_size * settings->step_size; g.rs = prep.rs; g.log_det = prep.log_det; g.cons_term = prep.cons_term;
        if (prep.precond == 1) mi::settings::pad_table(prep.sinv_diag.data(), d, dK, 1.0, &tabs[3 * (size_t)dK]);
        else std::fill_n(&tabs[3 * (size_t)dK], d, prep.rs);
    }
    DevBuf tabs_dev;
    if ((rc = upload_padded(tabs_dev, tabs.data(), tabs.size(), tabs.size(), 1.0))) return rc;
    g.mass_tables = tabs_dev.as<double>(); g.diag_mass = prep.precond == 1;
    // a DENSE precond_mat: INV(M), CHOL_LOWER(M), M and (mala) INV(eps^2 M), transposed on the device -- the very matrices the literal kernel reads (lit_upload),
    // so the products of the route and of its replay take the oracle's matrices bit for bit
    mi::lit::LitParams lp{};
    LitDev ldev;
    if (prep.precond == 2) {
        rc = lit_upload(prep, (uint32_t)d, false, ldev, lp);
        if (rc) return rc;
        g.dense_mass = true; g.M_t = lp.Mfull; g.Lc_t = lp.Lchol; g.Minv_t = lp.Minv; g.Sinv_t = lp.Sinv;
    }
    // a draw is a handful of launches + one or two per gradient: replayed from a captured graph while a launch is short (few chains); at full size the queue runs ahead anyway
    // (per leapfrog step / mala draw: the gradient's products and, with a dense precond_mat, one / five with the mass matrices)
    g.use_graph = ((double)d * (double)(logit ? 2 * n : d) + (g.dense_mass ? (algo == 0 ? 1.0 : 5.0) * (double)d * (double)d : 0.0)) * (double)C < 3.0e10
                  && g_gemm_graph_mode.load(std::memory_order_relaxed) == 0;      // (the test hook: never capture)
    const bool replay = algo != 3;                       // rwmh forms no product with a vector that can be non-finite (rwmh.cpp:126)
    WsLease base;
    ReplayWs rp = replay_layout(mi::gemm::gemm_ws_bytes((uint32_t)d, (uint32_t)n, C, g.dense_mass, bounded), C, (uint32_t)d, (uint32_t)(logit ? n : d), false);
    rc = ws_get(st, replay ? rp.total_bytes : rp.own_bytes, base);
    if (rc) return rc;
    if (replay) {
        rc = replay_bind(rp, base.p, C, st);
        if (rc) return rc;
        g.nf_flag = rp.flag;
    }
    g.ws = base.p;
    const char* kname = nullptr;
    const int e = mi::gemm::gemm_run(g, st, &kname);
    if (e != 0) return fail(MI_ERR_HIP, "%s: matrix-product sampler: %s", who, hipGetErrorString((hipError_t)e));
    if (replay) {                                        // chains that reached the non-finite regime: replayed literally (literal.hpp)
        if ((rc = lit_staged_target(lp.t, tg, (uint32_t)d, rp.tbuf, st))) return rc;
        lit_common(lp, settings, &sc.dev, rp, false);
        lp.rs = g.rs; lp.log_det = g.log_det; lp.cons_term = g.cons_term;
        if (prep.precond == 1) { lp.precond = 1; lp.m = g.mass_tables; lp.m_sqrt = g.mass_tables + dK; lp.m_inv = g.mass_tables + 2 * (size_t)dK; lp.sinv_diag = g.mass_tables + 3 * (size_t)dK; }
        if (bounded) { lp.vals_bound = 1; lp.btype = g.btype; lp.lb = g.lb; lp.ub = g.ub; }      // (the replay starts from theta, the untouched initial values: it transforms them itself)
        rc = launched("matrix-product sampler (literal replay)", mi::launch_literal(algo, lp, rp.n_wg, st));
        if (rc) return rc;
    }
    mi::note_kernel("%s", kname);
    return finish(chains, d, settings, sc, st, algo == 0 ? hmc_leap_total(settings) : 0, true);      // (the mass tables are ours)
}

// The one-lane-per-chain engine (rmhmc_small.hpp, small_samplers.hpp): hmc, mala, rwmh with any precond_mat / cov_mat and any
// bounds, nuts, rmhmc, for a target policy of dimension d <= SMALL_MAX_D.  Validates, stages the chains, packs the launch
// parameters; `launch` instantiates the kernels for its target type (the built-in policies below, or a user's library through
// mi_mcmc_run_user_target).  algo: 0 hmc, 1 mala, 2 nuts, 3 rwmh, 4 rmhmc.
int run_small(const char* who, int algo, uint64_t d, const mi_settings* settings, mi_chains* chains, hipStream_t st,
              const std::function<int(const mi::SmallParams&, hipStream_t)>& launch)
{
    if (d == 0 || d > (uint64_t)mi::SMALL_MAX_D) return fail(MI_ERR_UNSUPPORTED, "%s: the one-lane-per-chain engine takes 1 <= d <= %d", who, (int)mi::SMALL_MAX_D);
    if (settings->vals_bound && (!settings->lower_bounds || !settings->upper_bounds))
        return fail(MI_ERR_BAD_ARG, "%s: vals_bound needs lower_bounds and upper_bounds", who);
    const uint64_t n_total = settings->n_burnin_draws + settings->n_keep_draws;
    if (n_total > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "too many draws");
    if (algo == 2) {
        if (settings->max_tree_depth > (uint64_t)mi::NUTS_SMALL_MAX_DEPTH)
            return fail(MI_ERR_UNSUPPORTED, "nuts: max_tree_depth > %d not implemented for this target", (int)mi::NUTS_SMALL_MAX_DEPTH);
    }
    StagedChains sc;
    int rc = stage_in(chains, d, settings->n_keep_draws, sc, st, n_total);
    if (rc) return rc;

    mi::SmallParams prm{};
    fill_common(prm, d, settings, chains, sc);
    prm.n_leap = sc.dev.n_leapfrogs;
    prm.n_leap_steps = (uint32_t)settings->n_leap_steps; prm.n_fp_steps = (uint32_t)settings->n_fp_steps;
    prm.eps = settings->step_size;
    prm.vals_bound = settings->vals_bound ? 1 : 0;
    for (int i = 0; i < mi::SMALL_MAX_D; ++i)
        for (int k = 0; k < mi::SMALL_MAX_D; ++k) prm.M[i][k] = (i == k) ? 1.0 : 0.0;
    if (settings->precond_mat && algo != 4)          // hmc.cpp:57, mala.cpp:57, rwmh.cpp:58 (rmhmc has none)
        for (uint64_t i = 0; i < d; ++i)
            for (uint64_t k = 0; k < d; ++k) prm.M[i][k] = settings->precond_mat[i * d + k];
    mi::settings::bounds_tables(d, prm.vals_bound, settings->lower_bounds, settings->upper_bounds, prm.btype, prm.lb, prm.ub);
    mi::settings::pad_table(prm.btype, d, mi::SMALL_MAX_D, 1, prm.btype);      // (prm{}: lb and ub are zeros beyond d already)
    if (algo == 2 && (rc = fill_nuts(prm, settings, chains, sc))) return rc;
    rc = launched(who, launch(prm, st));
    if (rc) return rc;
    return finish(chains, d, settings, sc, st, NO_LEAP_FILL, false, n_total);
}

// the d = 2 normal model of the reference's example programs (MI_TARGET_NORMAL_MODEL)
int run_small_normal_model(const char* who, int algo, const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st)
{
    if (target->d != 2) return fail(MI_ERR_BAD_ARG, "%s: NORMAL_MODEL has d = 2 (mu, sigma)", who);
    if (!target->y || target->n_rows == 0 || target->n_rows > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "NORMAL_MODEL needs its observations in y[0..n_rows)");
    DevBuf x_owned;
    const double* x_dev = target->y;
    if (target->mem == MI_MEM_HOST) {
        HIP_TRY(x_owned.alloc(target->n_rows * sizeof(double)));
        HIP_TRY(hipMemcpy(x_owned.p, target->y, target->n_rows * sizeof(double), hipMemcpyHostToDevice));
        x_dev = x_owned.as<double>();
    }
    const uint32_t n_rows = (uint32_t)target->n_rows;
    const int rc = run_small(who, algo, 2, settings, chains, st, [&](const mi::SmallParams& p, hipStream_t s_) {
        mi::SmallParams q = p; q.data = x_dev; q.n_rows = n_rows;
        return mi::launch_small_normal_model(algo, q, s_);
    });
    if (rc) return rc;
    if (x_owned.p) HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

// Logistic regression with d <= SMALL_MAX_D coefficients on the one-lane-per-chain engine (small_targets.hpp: the bits of
// logit_lds_kernel): what the LDS kernel does not implement -- nuts, vals_bound, precond_mat / cov_mat
int run_small_logistic(const char* who, int algo, const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st)
{
    const uint64_t d = target->d;
    StagedTarget tg;
    int rc = stage_target(target, tg, st, 0xffffffffULL);
    if (rc) return rc;
    if (d > (uint64_t)mi::SMALL_MAX_D)
        return fail(MI_ERR_UNSUPPORTED, "%s: nuts / vals_bound / precond_mat / cov_mat on the logistic target are implemented for d <= %d "
                                        "(one chain per lane); d = %llu", who, (int)mi::SMALL_MAX_D, (unsigned long long)d);
    rc = run_small(who, algo, d, settings, chains, st, [&](const mi::SmallParams& p, hipStream_t s_) {
        return mi::launch_small_logistic(algo, (int)d, p, tg.mat, tg.y, (uint32_t)tg.n_rows, s_);
    });
    if (rc) return rc;
    if (tg.owns()) HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

}  // namespace

namespace mi {
namespace host {

// One chain of `algo` (0 hmc, 1 mala, 2 nuts, 3 rwmh, 4 rmhmc) on the literal kernel with the HOST callbacks as target (LIT_CALLBACK,
// literal.hpp): what mi_mcmc_rmhmc_run_callback is, and what the callback routes of the other samplers use for everything their
// host-driven form does not implement (bounds, precond_mat / cov_mat, max_tree_depth > 10).  This thread serves the kernel's requests.
int literal_run_callback(const char* who, int algo, const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel, void* target_data,
                         mi_tensor_cb tensor_fn, void* tensor_data, const mi_settings* settings, double* draws_out,
                         uint64_t* n_accept_draws, double* step_size_out)
{
    if (!initial_vals || !target_log_kernel || !settings) return fail(MI_ERR_BAD_ARG, "%s (callback): null initial_vals / callback / settings", who);
    if (settings->struct_size != sizeof(mi_settings)) return fail(MI_ERR_BAD_ARG, "struct_size mismatch");
    if (d == 0 || d > 0x7fffffffULL) return fail(MI_ERR_BAD_ARG, "%s (callback): d out of range", who);
    if (algo == 4 && d > (uint64_t)mi::lit::LIT_RMHMC_MAX_D)
        return fail(MI_ERR_UNSUPPORTED, "rmhmc (callback): d = %llu outside 1 .. %d (two d x d x d derivative cubes per chain)", (unsigned long long)d, (int)mi::lit::LIT_RMHMC_MAX_D);
    if (settings->vals_bound && (!settings->lower_bounds || !settings->upper_bounds)) return fail(MI_ERR_BAD_ARG, "%s (callback): vals_bound needs lower_bounds and upper_bounds", who);
    const bool mala_bounded = algo == 1 && settings->vals_bound != 0;
    if (mala_bounded && d > 512) return fail(MI_ERR_UNSUPPORTED, "mala (callback): vals_bound with d > 512 is not implemented (ten d x d matrices per workgroup)");
    if (algo == 2 && settings->max_tree_depth > (uint64_t)mi::lit::LIT_NUTS_MAX_DEPTH)
        return fail(MI_ERR_UNSUPPORTED, "nuts (callback): max_tree_depth > %d not implemented", (int)mi::lit::LIT_NUTS_MAX_DEPTH);
    const uint64_t n_keep = settings->n_keep_draws, n_total = settings->n_burnin_draws + n_keep;
    if (n_total > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "too many draws");
    if (n_keep > 0 && !draws_out) return fail(MI_ERR_BAD_ARG, "%s (callback): draws_out is required", who);
    if (int rc_dev = need_device()) return rc_dev;
    const size_t dd = (size_t)d * d;
    PinnedBuf ctl, val, xb, outb;
    HIP_TRY(ctl.alloc(mi::lit::LIT_MB_WORDS * sizeof(uint32_t))); HIP_TRY(val.alloc(8)); HIP_TRY(xb.alloc(d * 8));
    HIP_TRY(outb.alloc((algo == 4 ? dd + dd * d : d) * 8));
    std::memset(ctl.p, 0, mi::lit::LIT_MB_WORDS * sizeof(uint32_t));
    mi::lit::LitParams lp{};
    lp.t.kind = mi::lit::LIT_CALLBACK; lp.t.d = (uint32_t)d;
    mi::lit::lit_orders(lp.t);
    lp.t.mb.ctl = ctl.as<uint32_t>(); lp.t.mb.value = val.as<double>(); lp.t.mb.x = xb.as<double>(); lp.t.mb.out = outb.as<double>();
    lp.t.mb.timeout_ticks = 60ull * 100000000ull;          // 60 s of the 100 MHz wall clock per request
    DevBuf theta, draws, nacc, work, step;
    HIP_TRY(theta.alloc(d * 8)); HIP_TRY(draws.alloc(n_keep * d * 8)); HIP_TRY(nacc.alloc(8)); HIP_TRY(step.alloc(8));
    const size_t stride = mi::lit::lit_work_doubles((uint32_t)d, 0, mala_bounded, (uint32_t)settings->max_tree_depth, algo == 2, algo == 4);
    HIP_TRY(work.alloc(stride * 8));
    HIP_TRY(hipMemcpy(theta.p, initial_vals, d * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(nacc.p, 0, 8)); HIP_TRY(hipMemset(step.p, 0, 8));
    HIP_TRY(hipDeviceSynchronize());     // the kernel runs on its own NON-BLOCKING stream, which does not order itself behind the null stream's memsets / copies
    lp.C = 1; lp.chain0 = 0; lp.theta = theta.as<double>(); lp.draws = n_keep ? draws.as<double>() : nullptr; lp.n_accept = nacc.as<uint64_t>();
    lp.seed = settings->rng_seed_value;
    lp.n_burnin = (uint32_t)settings->n_burnin_draws; lp.n_keep = (uint32_t)n_keep; lp.n_leap_steps = (uint32_t)settings->n_leap_steps;
    lp.eps = settings->step_size; lp.n_fp_steps = (uint32_t)settings->n_fp_steps;
    lp.work = work.as<double>(); lp.work_stride = stride;
    if (algo == 2) {
        lp.n_adapt = (uint32_t)(settings->n_adapt_draws > n_total ? n_total : settings->n_adapt_draws);
        lp.max_depth = (uint32_t)settings->max_tree_depth;
        lp.delta = settings->target_accept_rate; lp.gamma = settings->gamma_val; lp.t0 = settings->t0_val; lp.kappa = settings->kappa_val;
        lp.step_out = step.as<double>();
    }
    mi::lit::LitPrep prep;
    int rc = mi::lit::lit_prepare(algo == 1 ? 1 : 0, (uint32_t)d, settings->step_size, settings->vals_bound ? 1 : 0, settings->lower_bounds, settings->upper_bounds,
                                  algo == 4 ? nullptr : settings->precond_mat, prep);
    if (rc) return rc;
    LitDev ldev;
    rc = lit_upload(prep, (uint32_t)d, settings->vals_bound != 0, ldev, lp);
    if (rc) return rc;
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    rc = launched(who, mi::launch_literal(algo, lp, 1, st));
    if (!rc) {
        (void)serve_callbacks(lp.t.mb, (uint32_t)d, target_log_kernel, target_data, tensor_fn, tensor_data, st);
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(MI_ERR_HIP, "%s (callback): %s", who, hipGetErrorString(e));
        else if (ctl.as<uint32_t>()[mi::lit::LIT_MB_ABORT] != 0u) rc = fail(MI_ERR_HIP, "%s (callback): the kernel gave up waiting for a callback (60 s)", who);
    }
    (void)hipStreamDestroy(st);
    if (rc) return rc;
    std::vector<double> rows(n_keep * d);
    if (n_keep) HIP_TRY(hipMemcpy(rows.data(), draws.p, n_keep * d * 8, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n_keep; ++i)
        for (uint64_t j = 0; j < d; ++j) draws_out[i + j * n_keep] = rows[i * d + j];       // column-major n_keep x d, as Eigen's Mat_t stores draws_out
    if (n_accept_draws) HIP_TRY(hipMemcpy(n_accept_draws, nacc.p, 8, hipMemcpyDeviceToHost));
    if (step_size_out && algo == 2) HIP_TRY(hipMemcpy(step_size_out, step.p, 8, hipMemcpyDeviceToHost));
    return MI_OK;
}


// ---- mcmc::de (src/de.cpp:28-232) for many populations: de.hpp.  Arguments are checked before anything touches the device.
int de_check(const char* who, uint64_t d, const mi_settings* s, const mi_de_settings* de, uint64_t draw0)
{
    if (!s || !de) return fail(MI_ERR_BAD_ARG, "%s: null settings / de_settings", who);
    if (s->struct_size != sizeof(mi_settings) || de->struct_size != sizeof(mi_de_settings))
        return fail(MI_ERR_BAD_ARG, "struct_size mismatch (header / library version skew)");
    if (d == 0 || d > 0x7fffffffULL) return fail(MI_ERR_BAD_ARG, "%s: d out of range", who);
    if (de->n_pop < 3) return fail(MI_ERR_BAD_ARG, "%s: n_pop = %llu; differential evolution needs n_pop >= 3 (the reference loops forever below)", who,
                                   (unsigned long long)de->n_pop);
    if (de->n_pop * (uint64_t)mi::de_blocks((uint32_t)d) >= (1ull << 32))
        return fail(MI_ERR_UNSUPPORTED, "%s: n_pop * (1 + ceil(d / 2)) >= 2^32 overflows the Philox slot counter", who);
    if (draw0 + s->n_burnin_draws + s->n_keep_draws > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: draw0 + generations exceeds the 32-bit counter", who);
    if (s->vals_bound && (!s->lower_bounds || !s->upper_bounds)) return fail(MI_ERR_BAD_ARG, "%s: vals_bound needs lower_bounds and upper_bounds", who);
    return MI_OK;
}

// the host-side half of DeParams: bounds (lit_prepare's tables), the initial box, gamma, counters
struct DeTables { mi::lit::LitPrep prep; LitDev ldev; DevBuf box_lb, box_ub; };
int de_tables(uint64_t d, const mi_settings* s, const mi_de_settings* de, DeTables& t, mi::DeParams& prm)
{
    int rc = mi::lit::lit_prepare(0, (uint32_t)d, 1.0, s->vals_bound ? 1 : 0, s->lower_bounds, s->upper_bounds, nullptr, t.prep);
    if (rc) return rc;
    if ((rc = lit_upload(t.prep, (uint32_t)d, s->vals_bound != 0, t.ldev, prm.lit))) return rc;
    if (de->initial_lb) {
        HIP_TRY(t.box_lb.alloc(d * 8)); HIP_TRY(hipMemcpy(t.box_lb.p, de->initial_lb, d * 8, hipMemcpyHostToDevice));
        prm.box_lb = t.box_lb.as<double>();
    }
    if (de->initial_ub) {
        HIP_TRY(t.box_ub.alloc(d * 8)); HIP_TRY(hipMemcpy(t.box_ub.p, de->initial_ub, d * 8, hipMemcpyHostToDevice));
        prm.box_ub = t.box_ub.as<double>();
    }
    prm.d = (uint32_t)d; prm.n_pop = (uint32_t)de->n_pop;
    prm.seed = s->rng_seed_value;
    prm.n_burnin = (uint32_t)s->n_burnin_draws; prm.n_keep = (uint32_t)s->n_keep_draws;
    prm.gamma = 2.38 / std::sqrt(2.0 * (double)d);         // de.cpp:61-62: par_gamma is not read
    prm.gamma_jump = de->par_gamma_jump; prm.b = de->par_b; prm.jumps = de->jumps ? 1 : 0;
    return MI_OK;
}

int de_run(const mi_target* target, const mi_settings* settings, const mi_de_settings* de, mi_populations* pops, hipStream_t st)
{
    if (!target || !pops) return fail(MI_ERR_BAD_ARG, "de: null target / populations");
    if (target->struct_size != sizeof(mi_target) || pops->struct_size != sizeof(mi_populations))
        return fail(MI_ERR_BAD_ARG, "struct_size mismatch (header / library version skew)");
    const uint64_t d = target->d, NP = pops->n_populations;
    int rc = de_check("de", d, settings, de, pops->draw0);
    if (rc) return rc;
    if (NP == 0) return fail(MI_ERR_BAD_ARG, "de: n_populations must be positive");
    if (!pops->population) return fail(MI_ERR_BAD_ARG, "de: populations.population is required");
    if (pops->draw0 == 0 && (!de->initial_lb || !de->initial_ub) && !pops->initial_vals)
        return fail(MI_ERR_BAD_ARG, "de: populations.initial_vals is required (a fresh run without de.initial_lb / initial_ub)");
    if (target->kind == MI_TARGET_NORMAL_MODEL)
        return fail(MI_ERR_UNSUPPORTED, "de: MI_TARGET_NORMAL_MODEL has no literal (one workgroup per population) evaluation, which the de kernels are built on");
    if (target->kind < MI_TARGET_GAUSS_ISO || target->kind > MI_TARGET_LOGISTIC) return fail(MI_ERR_UNSUPPORTED, "de: target kind %d not implemented", target->kind);
    if (int rc_dev = need_device()) return rc_dev;

    const uint64_t n_pop = de->n_pop, n_keep = settings->n_keep_draws;
    const size_t pop_doubles = (size_t)n_pop * d * NP;
    mi::DeParams prm{};
    DeTables tb;
    if ((rc = de_tables(d, settings, de, tb, prm))) return rc;
    prm.NP = NP; prm.pop0 = pops->population0; prm.draw0 = (uint32_t)pops->draw0;
    // populations in host memory are staged
    const bool host = pops->mem == MI_MEM_HOST;
    DevBuf s_init, s_pop, s_draws, s_acc;
    prm.init_vals = pops->initial_vals; prm.X = pops->population; prm.draws = pops->draws; prm.n_accept = pops->n_accept;
    if (host) {
        if (pops->initial_vals && pops->draw0 == 0) {
            HIP_TRY(s_init.alloc(d * NP * 8));
            HIP_TRY(hipMemcpyAsync(s_init.p, pops->initial_vals, d * NP * 8, hipMemcpyHostToDevice, st));
            prm.init_vals = s_init.as<double>();
        } else prm.init_vals = nullptr;
        HIP_TRY(s_pop.alloc(pop_doubles * 8));
        if (pops->draw0 > 0) HIP_TRY(hipMemcpyAsync(s_pop.p, pops->population, pop_doubles * 8, hipMemcpyHostToDevice, st));
        prm.X = s_pop.as<double>();
        if (pops->draws) { HIP_TRY(s_draws.alloc(n_keep * pop_doubles * 8)); prm.draws = s_draws.as<double>(); }
        if (pops->n_accept) { HIP_TRY(s_acc.alloc(NP * 8)); prm.n_accept = s_acc.as<uint64_t>(); }
    }
    const bool tile = (target->kind == MI_TARGET_GAUSS_ISO || target->kind == MI_TARGET_GAUSS_DIAG || target->kind == MI_TARGET_GAUSS_DENSE) &&
                      d <= 128 && target->kernel_hint != MI_KERNEL_LITERAL;
    DevBuf P_owned, t_a, t_b, t_t;
    unsigned n_wg = 0;
    size_t stride = 0;
    if (tile) {
        if ((rc = dense_precision_on_device(target, P_owned, &prm.P, st))) return rc;
    } else {
        if ((rc = lit_stage_target("de", target, prm.lit.t, t_a, t_b, t_t, st))) return rc;
        stride = mi::lit::lit_work_doubles((uint32_t)d, prm.lit.t.n_rows, false);
        n_wg = (unsigned)std::min<uint64_t>(NP, 1024u);
    }
    const size_t tv_bytes = ((size_t)n_pop * NP * 8 + 255) & ~(size_t)255;
    WsLease ws;
    if ((rc = ws_get(st, tv_bytes + (size_t)n_wg * stride * 8, ws))) return rc;
    prm.tv = ws.as<double>();
    prm.lit.work = reinterpret_cast<double*>(ws.as<char>() + tv_bytes); prm.lit.work_stride = stride;
    if (tile) rc = launched("de", mi::launch_de_gauss(prm, (int)((d + 15) / 16), settings->vals_bound != 0, st));
    else rc = launched("de", mi::launch_de_literal(prm, n_wg, st));
    if (rc) return rc;
    if (host) {
        HIP_TRY(hipMemcpyAsync(pops->population, prm.X, pop_doubles * 8, hipMemcpyDeviceToHost, st));
        if (pops->draws) HIP_TRY(hipMemcpyAsync(pops->draws, prm.draws, n_keep * pop_doubles * 8, hipMemcpyDeviceToHost, st));
        if (pops->n_accept) HIP_TRY(hipMemcpyAsync(pops->n_accept, prm.n_accept, NP * 8, hipMemcpyDeviceToHost, st));
    }
    if (host || P_owned.p || t_a.p || t_b.p || t_t.p || tb.ldev.any || tb.box_lb.p || tb.box_ub.p) HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

// one population on de_literal_kernel with the HOST callback as target (LIT_CALLBACK): this thread serves the kernel's requests
int de_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel, void* target_data, const mi_settings* settings,
                    const mi_de_settings* de, double* draws_out, uint64_t* n_accept)
{
    if (!initial_vals || !target_log_kernel) return fail(MI_ERR_BAD_ARG, "de (callback): null initial_vals / callback");
    int rc = de_check("de (callback)", d, settings, de, 0);
    if (rc) return rc;
    const uint64_t n_pop = de->n_pop, n_keep = settings->n_keep_draws;
    if (n_keep > 0 && !draws_out) return fail(MI_ERR_BAD_ARG, "de (callback): draws_out is required");
    if (int rc_dev = need_device()) return rc_dev;
    PinnedBuf ctl, val, xb, outb;
    HIP_TRY(ctl.alloc(mi::lit::LIT_MB_WORDS * sizeof(uint32_t))); HIP_TRY(val.alloc(8)); HIP_TRY(xb.alloc(d * 8)); HIP_TRY(outb.alloc(d * 8));
    std::memset(ctl.p, 0, mi::lit::LIT_MB_WORDS * sizeof(uint32_t));
    mi::DeParams prm{};
    prm.lit.t.kind = mi::lit::LIT_CALLBACK; prm.lit.t.d = (uint32_t)d;
    mi::lit::lit_orders(prm.lit.t);
    mi::lit::LitMailbox& mb = prm.lit.t.mb;
    mb.ctl = ctl.as<uint32_t>(); mb.value = val.as<double>(); mb.x = xb.as<double>(); mb.out = outb.as<double>();
    mb.timeout_ticks = 60ull * 100000000ull;              // 60 s of the 100 MHz wall clock per request
    DeTables tb;
    if ((rc = de_tables(d, settings, de, tb, prm))) return rc;
    const size_t pop_doubles = (size_t)n_pop * d;
    const size_t stride = mi::lit::lit_work_doubles((uint32_t)d, 0, false);
    DevBuf init, X, tv, draws, acc, work;
    HIP_TRY(init.alloc(d * 8)); HIP_TRY(X.alloc(pop_doubles * 8)); HIP_TRY(tv.alloc(n_pop * 8));
    HIP_TRY(draws.alloc(n_keep * pop_doubles * 8)); HIP_TRY(acc.alloc(8)); HIP_TRY(work.alloc(stride * 8));
    HIP_TRY(hipMemcpy(init.p, initial_vals, d * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(acc.p, 0, 8));
    HIP_TRY(hipDeviceSynchronize());     // the kernel runs on its own NON-BLOCKING stream, which does not order itself behind the null stream's copies
    prm.NP = 1; prm.pop0 = 0; prm.draw0 = 0;
    prm.init_vals = init.as<double>(); prm.X = X.as<double>(); prm.tv = tv.as<double>();
    prm.draws = n_keep ? draws.as<double>() : nullptr; prm.n_accept = acc.as<uint64_t>();
    prm.lit.work = work.as<double>(); prm.lit.work_stride = stride;
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    rc = launched("de (callback)", mi::launch_de_literal(prm, 1, st));
    if (!rc) {
        (void)serve_callbacks(mb, (uint32_t)d, target_log_kernel, target_data, nullptr, nullptr, st);
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(MI_ERR_HIP, "de (callback): %s", hipGetErrorString(e));
        else if (ctl.as<uint32_t>()[mi::lit::LIT_MB_ABORT] != 0u) rc = fail(MI_ERR_HIP, "de (callback): the kernel gave up waiting for a callback (60 s)");
    }
    (void)hipStreamDestroy(st);
    if (rc) return rc;
    if (n_keep) HIP_TRY(hipMemcpy(draws_out, draws.p, n_keep * pop_doubles * 8, hipMemcpyDeviceToHost));
    if (n_accept) HIP_TRY(hipMemcpy(n_accept, acc.p, 8, hipMemcpyDeviceToHost));
    return MI_OK;
}


// ---- mcmc::aees (src/aees.cpp:28-305) for many runs: aees.hpp.  Arguments are checked before anything touches the device.
#ifndef MI_AEES_WS_MAX_BYTES
#define MI_AEES_WS_MAX_BYTES ((size_t)16 << 30)          // the history slots of one call: runs beyond what fits wait for a free slot
#endif
constexpr unsigned AEES_MAX_WG = 2048;                   // 8 workgroups of 256 threads per CU on 256 CUs

int aees_check(const char* who, uint64_t d, const mi_settings* s, const mi_aees_settings* a)
{
    if (!s || !a) return fail(MI_ERR_BAD_ARG, "%s: null settings / aees_settings", who);
    if (s->struct_size != sizeof(mi_settings) || a->struct_size != sizeof(mi_aees_settings))
        return fail(MI_ERR_BAD_ARG, "struct_size mismatch (header / library version skew)");
    if (d == 0 || d > 0x7fffffffULL) return fail(MI_ERR_BAD_ARG, "%s: d out of range", who);
    if (a->n_rings == 0) return fail(MI_ERR_BAD_ARG, "%s: n_rings = 0 (the reference's n_rings - 1 wraps)", who);
    if (a->temper_len > 0 && !a->temper_vec) return fail(MI_ERR_BAD_ARG, "%s: temper_len > 0 needs temper_vec", who);
    if (a->temper_len > 0xffffULL) return fail(MI_ERR_BAD_ARG, "%s: temper_len out of range", who);
    for (uint64_t i = 0; i < a->temper_len; ++i)
        if (!(a->temper_vec[i] > 0.0) || !std::isfinite(a->temper_vec[i]))
            return fail(MI_ERR_BAD_ARG, "%s: temper_vec[%llu] = %g: every temperature must be finite and > 0", who, (unsigned long long)i, a->temper_vec[i]);
    const unsigned __int128 K = (unsigned __int128)a->temper_len + 1;
    const unsigned __int128 n_total = (unsigned __int128)s->n_keep_draws + K * ((unsigned __int128)a->n_initial_draws + s->n_burnin_draws);
    if (n_total >= ((unsigned __int128)1 << 32)) return fail(MI_ERR_BAD_ARG, "%s: n_keep + K (n_initial + n_burnin) must stay below 2^32", who);
    if (s->vals_bound && (!s->lower_bounds || !s->upper_bounds)) return fail(MI_ERR_BAD_ARG, "%s: vals_bound needs lower_bounds and upper_bounds", who);
    return MI_OK;
}

// the host-side half of AeesParams: bounds, the temperatures (descending), the K scaled proposal matrices
struct AeesTables { mi::lit::LitPrep prep; LitDev ldev; DevBuf temp, At; };
int aees_tables(uint64_t d, const mi_settings* s, const mi_aees_settings* a, AeesTables& t, mi::AeesParams& prm)
{
    int rc = mi::lit::lit_prepare(0, (uint32_t)d, 1.0, s->vals_bound ? 1 : 0, s->lower_bounds, s->upper_bounds, nullptr, t.prep);
    if (rc) return rc;
    if ((rc = lit_upload(t.prep, (uint32_t)d, s->vals_bound != 0, t.ldev, prm.lit))) return rc;
    const uint32_t K = (uint32_t)a->temper_len + 1;
    std::vector<double> T(a->temper_vec, a->temper_vec + a->temper_len);
    T.push_back(1.0);                                       // aees.cpp:62-76: 1 appended, sorted descending
    std::sort(T.begin(), T.end(), [](double x, double y) { return x > y; });
    std::vector<double> L((size_t)d * d, 0.0);              // CHOL_LOWER(cov_mat), or the identity (aees.cpp:82-85)
    if (a->cov_mat) {
        std::vector<double> Lc;
        if ((rc = host_cholesky_lower(a->cov_mat, (size_t)d, Lc))) return rc;
        L = Lc;
    } else for (uint64_t i = 0; i < d; ++i) L[i * d + i] = 1.0;
    std::vector<double> At((size_t)K * d * d);              // (sqrt(T_k) * (par_scale * L)), transposed per level
    for (uint32_t k = 0; k < K; ++k) {
        const double sq = std::sqrt(T[k]);
        for (uint64_t i = 0; i < d; ++i)
            for (uint64_t c = 0; c < d; ++c) At[((size_t)k * d + c) * d + i] = sq * (a->par_scale * L[i * d + c]);
    }
    HIP_TRY(t.temp.alloc(K * 8)); HIP_TRY(hipMemcpy(t.temp.p, T.data(), K * 8, hipMemcpyHostToDevice));
    HIP_TRY(t.At.alloc(At.size() * 8)); HIP_TRY(hipMemcpy(t.At.p, At.data(), At.size() * 8, hipMemcpyHostToDevice));
    prm.d = (uint32_t)d; prm.K = K; prm.n_rings = a->n_rings;
    prm.S = (uint32_t)(a->n_initial_draws + s->n_burnin_draws); prm.n_keep = (uint32_t)s->n_keep_draws;
    prm.n_total = prm.n_keep + K * prm.S;
    prm.seed = s->rng_seed_value; prm.ee_prob = a->ee_prob_par;
    prm.temp = t.temp.as<double>(); prm.At = t.At.as<double>();
    return MI_OK;
}

// the workgroups of one launch and their workspace: literal scratch + one history slot each
int aees_workspace(mi::AeesParams& prm, uint64_t n_runs, hipStream_t st, WsLease& ws, unsigned& n_wg)
{
    const size_t slot = mi::aees_slot_bytes(prm.d, prm.K, prm.S, prm.n_total);
    prm.lit_stride = mi::lit::lit_work_doubles(prm.d, prm.lit.t.n_rows, false);
    const size_t work = ((mi::aees_work_doubles(prm.lit_stride, prm.d, prm.K) * 8) + 255) & ~(size_t)255;
    if (slot + work > MI_AEES_WS_MAX_BYTES)
        return fail(MI_ERR_OOM, "aees: one run's history needs %zu bytes, more than the %zu-byte budget", slot + work, (size_t)MI_AEES_WS_MAX_BYTES);
    n_wg = (unsigned)std::min<uint64_t>({n_runs, (uint64_t)AEES_MAX_WG, (uint64_t)(MI_AEES_WS_MAX_BYTES / (slot + work))});
    int rc = ws_get(st, (size_t)n_wg * (slot + work), ws);
    if (rc) return rc;
    prm.lit.work = ws.as<double>(); prm.lit.work_stride = work / 8;
    prm.hist = ws.as<char>() + (size_t)n_wg * work; prm.hist_stride = slot;
    return MI_OK;
}

int aees_run(const mi_target* target, const mi_settings* settings, const mi_aees_settings* aees, mi_aees_runs* runs, hipStream_t st)
{
    if (!target || !runs) return fail(MI_ERR_BAD_ARG, "aees: null target / runs");
    if (target->struct_size != sizeof(mi_target) || runs->struct_size != sizeof(mi_aees_runs))
        return fail(MI_ERR_BAD_ARG, "struct_size mismatch (header / library version skew)");
    const uint64_t d = target->d, P = runs->n_runs;
    int rc = aees_check("aees", d, settings, aees);
    if (rc) return rc;
    if (P == 0) return fail(MI_ERR_BAD_ARG, "aees: n_runs must be positive");
    if (!runs->initial_vals) return fail(MI_ERR_BAD_ARG, "aees: runs.initial_vals is required");
    if (target->kind == MI_TARGET_NORMAL_MODEL)
        return fail(MI_ERR_UNSUPPORTED, "aees: MI_TARGET_NORMAL_MODEL has no literal (one workgroup per run) evaluation, which the aees kernel is built on");
    if (target->kind < MI_TARGET_GAUSS_ISO || target->kind > MI_TARGET_GAUSS_MIXTURE) return fail(MI_ERR_UNSUPPORTED, "aees: target kind %d not implemented", target->kind);
    if (int rc_dev = need_device()) return rc_dev;

    mi::AeesParams prm{};
    AeesTables tb;
    if ((rc = aees_tables(d, settings, aees, tb, prm))) return rc;
    const uint64_t K = prm.K, n_keep = prm.n_keep;
    prm.P = P; prm.run0 = runs->run0; prm.r_begin = 0; prm.r_end = P;
    const bool host = runs->mem == MI_MEM_HOST;
    DevBuf s_init, s_draws, s_fin, s_acc, s_ee;
    prm.init = runs->initial_vals; prm.draws = runs->draws; prm.fin = runs->final_states; prm.n_acc = runs->n_accept; prm.n_ee = runs->n_ee_accept;
    if (host) {                                             // runs in host memory are staged
        HIP_TRY(s_init.alloc(d * P * 8));
        HIP_TRY(hipMemcpyAsync(s_init.p, runs->initial_vals, d * P * 8, hipMemcpyHostToDevice, st));
        prm.init = s_init.as<double>();
        if (runs->draws) { HIP_TRY(s_draws.alloc(n_keep * d * P * 8)); prm.draws = s_draws.as<double>(); }
        if (runs->final_states) { HIP_TRY(s_fin.alloc(K * d * P * 8)); prm.fin = s_fin.as<double>(); }
        if (runs->n_accept) { HIP_TRY(s_acc.alloc(K * P * 8)); prm.n_acc = s_acc.as<uint64_t>(); }
        if (runs->n_ee_accept) { HIP_TRY(s_ee.alloc(K * P * 8)); prm.n_ee = s_ee.as<uint64_t>(); }
    }
    DevBuf t_a, t_b, t_t;
    if ((rc = lit_stage_target("aees", target, prm.lit.t, t_a, t_b, t_t, st, true))) return rc;
    WsLease ws;
    unsigned n_wg = 0;
    if ((rc = aees_workspace(prm, P, st, ws, n_wg))) return rc;
    if ((rc = launched("aees", mi::launch_aees_literal(prm, n_wg, st)))) return rc;
    if (host) {
        if (runs->draws) HIP_TRY(hipMemcpyAsync(runs->draws, prm.draws, n_keep * d * P * 8, hipMemcpyDeviceToHost, st));
        if (runs->final_states) HIP_TRY(hipMemcpyAsync(runs->final_states, prm.fin, K * d * P * 8, hipMemcpyDeviceToHost, st));
        if (runs->n_accept) HIP_TRY(hipMemcpyAsync(runs->n_accept, prm.n_acc, K * P * 8, hipMemcpyDeviceToHost, st));
        if (runs->n_ee_accept) HIP_TRY(hipMemcpyAsync(runs->n_ee_accept, prm.n_ee, K * P * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));                      // the tables above are freed on return
    return MI_OK;
}

// one run on aees_literal_kernel with the HOST callback as target (LIT_CALLBACK): this thread serves the kernel's requests
int aees_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel, void* target_data, const mi_settings* settings,
                      const mi_aees_settings* aees, double* draws_out, double* final_states, uint64_t* n_accept, uint64_t* n_ee_accept)
{
    if (!initial_vals || !target_log_kernel) return fail(MI_ERR_BAD_ARG, "aees (callback): null initial_vals / callback");
    int rc = aees_check("aees (callback)", d, settings, aees);
    if (rc) return rc;
    const uint64_t n_keep = settings->n_keep_draws, K = aees->temper_len + 1;
    if (n_keep > 0 && !draws_out) return fail(MI_ERR_BAD_ARG, "aees (callback): draws_out is required");
    if (int rc_dev = need_device()) return rc_dev;
    PinnedBuf ctl, val, xb, outb;
    HIP_TRY(ctl.alloc(mi::lit::LIT_MB_WORDS * sizeof(uint32_t))); HIP_TRY(val.alloc(8)); HIP_TRY(xb.alloc(d * 8)); HIP_TRY(outb.alloc(d * 8));
    std::memset(ctl.p, 0, mi::lit::LIT_MB_WORDS * sizeof(uint32_t));
    mi::AeesParams prm{};
    prm.lit.t.kind = mi::lit::LIT_CALLBACK; prm.lit.t.d = (uint32_t)d;
    mi::lit::lit_orders(prm.lit.t);
    mi::lit::LitMailbox& mb = prm.lit.t.mb;
    mb.ctl = ctl.as<uint32_t>(); mb.value = val.as<double>(); mb.x = xb.as<double>(); mb.out = outb.as<double>();
    mb.timeout_ticks = 60ull * 100000000ull;              // 60 s of the 100 MHz wall clock per request
    AeesTables tb;
    if ((rc = aees_tables(d, settings, aees, tb, prm))) return rc;
    prm.lit_stride = mi::lit::lit_work_doubles((uint32_t)d, 0, false);
    const size_t slot = mi::aees_slot_bytes(prm.d, prm.K, prm.S, prm.n_total);
    const size_t work = mi::aees_work_doubles(prm.lit_stride, prm.d, prm.K);
    DevBuf init, draws, fin, acc, ee, wk, hist;
    HIP_TRY(init.alloc(d * 8)); HIP_TRY(draws.alloc(std::max<uint64_t>(n_keep, 1) * d * 8)); HIP_TRY(fin.alloc(K * d * 8));
    HIP_TRY(acc.alloc(K * 8)); HIP_TRY(ee.alloc(K * 8)); HIP_TRY(wk.alloc(work * 8)); HIP_TRY(hist.alloc(std::max<size_t>(slot, 256)));
    HIP_TRY(hipMemcpy(init.p, initial_vals, d * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());     // the kernel runs on its own NON-BLOCKING stream, which does not order itself behind the null stream's copies
    prm.P = 1; prm.run0 = 0; prm.r_begin = 0; prm.r_end = 1;
    prm.init = init.as<double>(); prm.draws = n_keep ? draws.as<double>() : nullptr; prm.fin = fin.as<double>();
    prm.n_acc = acc.as<uint64_t>(); prm.n_ee = ee.as<uint64_t>();
    prm.lit.work = wk.as<double>(); prm.lit.work_stride = work;
    prm.hist = hist.as<char>(); prm.hist_stride = slot;
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    rc = launched("aees (callback)", mi::launch_aees_literal(prm, 1, st));
    if (!rc) {
        (void)serve_callbacks(mb, (uint32_t)d, target_log_kernel, target_data, nullptr, nullptr, st);
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(MI_ERR_HIP, "aees (callback): %s", hipGetErrorString(e));
        else if (ctl.as<uint32_t>()[mi::lit::LIT_MB_ABORT] != 0u) rc = fail(MI_ERR_HIP, "aees (callback): the kernel gave up waiting for a callback (60 s)");
    }
    (void)hipStreamDestroy(st);
    if (rc) return rc;
    if (n_keep) HIP_TRY(hipMemcpy(draws_out, draws.p, n_keep * d * 8, hipMemcpyDeviceToHost));
    if (final_states) HIP_TRY(hipMemcpy(final_states, fin.p, K * d * 8, hipMemcpyDeviceToHost));
    if (n_accept) HIP_TRY(hipMemcpy(n_accept, acc.p, K * 8, hipMemcpyDeviceToHost));
    if (n_ee_accept) HIP_TRY(hipMemcpy(n_ee_accept, ee.p, K * 8, hipMemcpyDeviceToHost));
    return MI_OK;
}

}  // namespace host
}  // namespace mi

extern "C" {

void mi_settings_default(mi_settings* s)
{
    if (!s) return;
    std::memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(mi_settings);
    s->rng_seed_value = 0;
    s->n_burnin_draws = 1000;
    s->n_keep_draws = 1000;
    s->n_leap_steps = 1;
    s->step_size = 1.0;
    s->n_adapt_draws = 1000;
    s->target_accept_rate = 0.55;
    s->max_tree_depth = 10;
    s->gamma_val = 0.05;
    s->t0_val = 10.0;
    s->kappa_val = 0.75;
    s->n_fp_steps = 5;
}

const char* mi_mcmc_last_error(void) { return mi::host::last_error().c_str(); }
const char* mi_mcmc_last_kernel(void) { return mi::host::last_kernel().c_str(); }
int mi_mcmc_version(void) { return MI_MCMC_VERSION; }
int mi_mcmc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mi_mcmc_run_user_target(int algo, uint64_t d, mi_small_launch_fn launch, const void* target_pod, uint64_t small_params_bytes,
                            const mi_settings* settings, mi_chains* chains, void* stream)
{
    if (!launch || !settings || !chains) return fail(MI_ERR_BAD_ARG, "null launch / settings / chains");
    if (algo < 0 || algo > 4) return fail(MI_ERR_BAD_ARG, "algo: 0 hmc, 1 mala, 2 nuts, 3 rwmh, 4 rmhmc");
    if (small_params_bytes != sizeof(mi::SmallParams))
        return fail(MI_ERR_BAD_ARG, "the target library was built against another version of the engine headers (SmallParams %llu vs %llu bytes)",
                    (unsigned long long)small_params_bytes, (unsigned long long)sizeof(mi::SmallParams));
    if (settings->struct_size != sizeof(mi_settings) || chains->struct_size != sizeof(mi_chains))
        return fail(MI_ERR_BAD_ARG, "struct_size mismatch (header / library version skew)");
    if (chains->n_chains == 0 || !chains->theta) return fail(MI_ERR_BAD_ARG, "chains.theta and n_chains are required");
    if (int rc_dev = need_device()) return rc_dev;
    static const char* const names[5] = {"hmc", "mala", "nuts", "rwmh", "rmhmc"};
    return run_small(names[algo], algo, d, settings, chains, static_cast<hipStream_t>(stream), [&](const mi::SmallParams& p, hipStream_t s_) {
        return launch(algo, &p, target_pod, s_);
    });
}

int mi_mcmc_run_tile_target(int algo, uint64_t d, int nt, int wpb, uint64_t lds_bytes, mi_tile_launch_fn launch, const void* target_pod,
                            uint64_t tile_params_bytes, int header_version, const mi_settings* settings, mi_chains* chains, void* stream)
{
    if (!launch || !target_pod || !settings || !chains) return fail(MI_ERR_BAD_ARG, "null launch function / target / settings / chains");
    if (header_version != MI_MCMC_VERSION)
        return fail(MI_ERR_BAD_ARG, "the target library was built against engine headers %#x, this library is %#x: rebuild it", header_version, MI_MCMC_VERSION);
    if (tile_params_bytes != sizeof(mi::TileParams))
        return fail(MI_ERR_BAD_ARG, "the target library was built against another version of the engine headers (TileParams %llu vs %llu bytes)",
                    (unsigned long long)tile_params_bytes, (unsigned long long)sizeof(mi::TileParams));
    if (settings->struct_size != sizeof(mi_settings) || chains->struct_size != sizeof(mi_chains))
        return fail(MI_ERR_BAD_ARG, "struct_size mismatch (header / library version skew)");
    if (algo != 0 && algo != 1 && algo != 2) return fail(MI_ERR_UNSUPPORTED, "tile targets: hmc (0), mala (1) and nuts (2) are implemented");
    if (algo == 2 && settings->max_tree_depth > (uint64_t)mi::tile_nuts::NUTS_MAX_DEPTH)
        return fail(MI_ERR_UNSUPPORTED, "tile targets: nuts with max_tree_depth > %d is not implemented on this route", (int)mi::tile_nuts::NUTS_MAX_DEPTH);
    if (!(nt == 1 || nt == 2 || nt == 4 || nt == 8) || d == 0 || d > (uint64_t)16 * nt) return fail(MI_ERR_BAD_ARG, "tile targets: 1 <= d <= 16 NT, NT in {1, 2, 4, 8}");
    if (wpb != 4 && wpb != 8) return fail(MI_ERR_BAD_ARG, "tile targets: WPB is 4 or 8");
    // vals_bound and / or a DIAGONAL precond_mat: hmc and nuts (TileGen, tile_samplers.hpp); mala with a diagonal precond_mat alone (round 6:
    // mala_tile_kernel<T, true>).  mala with bounds and a dense precond_mat stay with the one-lane targets (include/mi_mcmc_target.hpp), which take
    // every combination: refused here with the reason
    GeneralTables gt;
    const bool mala_diag = algo == 1 && !settings->vals_bound && settings->precond_mat != nullptr;
    if (settings->vals_bound || settings->precond_mat) {
        if (algo == 1 && settings->vals_bound) return fail(MI_ERR_UNSUPPORTED, "tile targets: mala with vals_bound is not implemented on this route (one-lane targets, include/mi_mcmc_target.hpp, take it)");
        const int rcg = general_tables("tile targets", settings, d, gt, false);
        if (rcg) return rcg;
    }
    if (chains->n_chains == 0 || !chains->theta) return fail(MI_ERR_BAD_ARG, "chains.theta and n_chains are required");
    const uint64_t n_total = settings->n_burnin_draws + settings->n_keep_draws;
    if (chains->draw0 + n_total > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "draw0 + draws exceeds the 32-bit draw counter");
    if (int rc_dev = need_device()) return rc_dev;
    int dev = 0, lds_max = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    if (lds_bytes > (uint64_t)lds_max) return fail(MI_ERR_BAD_ARG, "tile targets: the target asks for %llu bytes of LDS, a workgroup has %d", (unsigned long long)lds_bytes, lds_max);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t lds_user = lds_bytes;
    if (algo == 2) lds_bytes += mi::tile_nuts::lds_doubles() * sizeof(double);     // the sampler's per-level tables behind the target's own LDS
    if (gt.active && !mala_diag) lds_bytes += (uint64_t)(16 * nt * 4 + 8 * nt) * sizeof(double);  // TileGen<NT>::lds_doubles(): bounds / mass tables
    if (mala_diag) lds_bytes += (uint64_t)(3 * 16 * nt) * sizeof(double);           // mala_tile_kernel<T, true>: m | sqrt(m) | 1 / (eps^2 m)
    if (lds_bytes > (uint64_t)lds_max) return fail(MI_ERR_BAD_ARG, "tile targets: target + nuts tables ask for %llu bytes of LDS, a workgroup has %d", (unsigned long long)lds_bytes, lds_max);
    StagedChains sc;
    int rc = stage_in(chains, d, settings->n_keep_draws, sc, st, n_total);
    if (rc) return rc;
    mi::TileParams p{};
    fill_common(p, d, settings, chains, sc);
    p.n_leap = sc.dev.n_leapfrogs;
    p.n_leap_steps = (uint32_t)settings->n_leap_steps;
    p.eps = settings->step_size;
    // Sigma = eps^2 M is constant: INV(Sigma) = diag(1 / (eps^2 m_i)) and LOG_DET(Sigma) as the oracle's Gauss-Jordan / Cholesky give them for the identity
    // or a diagonal matrix (settings_host.hpp: mala_sigma; the built-in general mala kernel, mala_dense.hpp, forms the same values)
    mi::settings::MalaSigma sg;
    (void)mi::settings::mala_sigma(d, settings->step_size, mala_diag ? 1 : 0, mala_diag ? gt.m.data() : nullptr, sg);
    p.s2 = settings->step_size * settings->step_size; p.rs = sg.rs; p.cons_term = sg.cons_term; p.log_det = sg.log_det;
    p.lds_user_doubles = (uint32_t)(lds_user / sizeof(double));
    DevBuf sinv_dev;
    if (mala_diag) {
        if ((rc = upload_padded(sinv_dev, sg.sinv_diag.data(), d, d, 1.0)) || (rc = gt.upload_m())) return rc;
        p.m = gt.m_dev.as<double>(); p.m_sqrt = gt.ms_dev.as<double>(); p.s_inv = sinv_dev.as<double>();
    }
    else if (gt.active) {
        p.vals_bound = settings->vals_bound ? 1 : 0;
        p.btype = gt.bt.as<int>(); p.lb = gt.lb.as<double>(); p.ub = gt.ub.as<double>();
        p.m_sqrt = gt.ms_dev.as<double>(); p.m_inv = gt.mi_dev.as<double>();
    }
    WsLease ws;
    if (algo == 2) {                                       // nuts: point records + scalar table of every chain slot (nuts_memo_core.hpp), one workgroup per 64 chains
        if ((rc = fill_nuts(p, settings, chains, sc))) return rc;
        p.eps_bar0 = settings->step_size;
        const int nt_pad = nt <= 1 ? 1 : nt == 2 ? 2 : nt <= 4 ? 4 : 8;
        // a persistent grid (one workgroup per CU at most) with the chains handed out dynamically: the workspace is sized by the grid's chain slots
        const uint64_t n_wg = mi::nuts_tile_grid(chains->n_chains);
        const size_t vec_bytes = (mi::tile_nuts::ws_bytes_grid(n_wg, nt_pad) + 255) & ~(size_t)255;
        const size_t split_bytes = chains->n_chains > n_wg * 64 ? mi::nuts_split_workspace_bytes(chains->n_chains, 0) : 0;     // (more chains than chain slots: the runs cut into pieces)
        rc = ws_get(st, vec_bytes + 256 + split_bytes, ws);
        if (rc) return rc;
        p.ws = ws.as<double>();
        p.nuts_grid = (uint32_t)n_wg;
        p.next_chain = reinterpret_cast<uint32_t*>(static_cast<char*>(ws.p) + vec_bytes);
        HIP_TRY(hipMemsetAsync(p.next_chain, 0, sizeof(uint32_t), st));
        p.n_exec = sc.dev.n_leapfrogs_executed; sc.exec_written = p.n_exec != nullptr;     // (each distinct state of a doubling is evaluated once)
        if (split_bytes) { const int e = mi::nuts_tile_setup_pieces(p, static_cast<char*>(ws.p) + vec_bytes + 256, st); if (e != 0) return fail(MI_ERR_HIP, "tile target nuts: %s", hipGetErrorString((hipError_t)e)); }
    } else {
        rc = ws_get(st, (size_t)3 * 16 * nt * ((chains->n_chains + 15) / 16 + 8) * 16 * sizeof(double), ws);
        if (rc) return rc;
        p.wsave = ws.as<double>();
    }
    mi::note_kernel("%s_tile%s_kernel<user target, %d>", algo == 0 ? "hmc" : algo == 1 ? "mala" : "nuts", gt.active ? "_gen" : "", (algo == 0 && !gt.active) ? wpb : 4);     // (mala_tile_gen: mala_tile_kernel<T, true>)
    const int e = launch(algo, &p, target_pod, lds_bytes, stream);
    if (e != 0) return fail(MI_ERR_HIP, "tile target kernel launch: %s", hipGetErrorString((hipError_t)e));
    return finish(chains, d, settings, sc, st, algo == 1 ? 0 : NO_LEAP_FILL, gt.active, n_total);      // (the tables are ours)
}

int mi_mcmc_run_user_target_v(int algo, uint64_t d, mi_small_launch_fn launch, const void* target_pod, uint64_t small_params_bytes,
                              int header_version, const mi_settings* settings, mi_chains* chains, void* stream)
{
    if (header_version != MI_MCMC_VERSION)
        return fail(MI_ERR_BAD_ARG, "the target library was built against engine headers %#x, this library is %#x: rebuild it", header_version, MI_MCMC_VERSION);
    return mi_mcmc_run_user_target(algo, d, launch, target_pod, small_params_bytes, settings, chains, stream);
}

int mi_mcmc_mat_inverse(const double* A, uint64_t d, double* Ainv)
{
    if (!A || !Ainv) return fail(MI_ERR_BAD_ARG, "mat_inverse: NULL matrix");
    if (linalg_on_device(0, (size_t)d) && mi_mcmc_device_count() < 1) return fail(MI_ERR_NO_DEVICE, "mat_inverse: no GPU visible (d >= 64 runs on the device)");
    std::vector<double> out;
    const int rc = host_inverse(A, (size_t)d, out);
    if (rc) return rc;
    std::memcpy(Ainv, out.data(), (size_t)d * d * sizeof(double));
    return MI_OK;
}

int mi_mcmc_mat_cholesky_lower(const double* A, uint64_t d, double* L)
{
    if (!A || !L) return fail(MI_ERR_BAD_ARG, "mat_cholesky_lower: NULL matrix");
    if (linalg_on_device(1, (size_t)d) && mi_mcmc_device_count() < 1) return fail(MI_ERR_NO_DEVICE, "mat_cholesky_lower: no GPU visible (d >= 64 runs on the device)");
    std::vector<double> out;
    const int rc = host_cholesky_lower(A, (size_t)d, out);
    if (rc) return rc;
    std::memcpy(L, out.data(), (size_t)d * d * sizeof(double));
    return MI_OK;
}

int mi_mcmc_release_workspace(void* stream, int all_streams, uint64_t* bytes_freed)
{
    linalg_memo_clear();         // the calling thread's two memoised inverses of a precond_mat (host_linalg.hpp: 2 MiB each at d = 512)
    return ws_release(static_cast<hipStream_t>(stream), all_streams != 0, bytes_freed);
}

// ---- the two Gaussian routes of mi_mcmc_hmc_run that are kernels of their own: the elementwise kernels (separable targets, any d) and the d <= 128 tile kernels
// (static, here and before the other entry points: inside extern "C" a function keeps its C name even in an unnamed namespace, and the library exports the ABI only)
namespace {
struct HmcGaussCase { bool dense_m, bounded, diag_precond_elementwise; };      // what the ladder has decided when it reaches them
// chains that reached the non-finite regime behind a plain launch: replayed literally (literal.hpp) with the same masses.  P_dense / prec_vec: lit_gauss_target
static int hmc_gauss_replay(const mi_target* target, const mi_settings* settings, const StagedChains& sc, const ReplayWs& rp, const double* P_dense, const double* prec_vec,
                     const HmcMass& hm, hipStream_t st)
{
    mi::lit::LitParams lp{};
    const int rc = lit_gauss_target(lp.t, target->kind, (uint32_t)target->d, P_dense, prec_vec, rp.tbuf, st);
    if (rc) return rc;
    lit_common(lp, settings, &sc.dev, rp, false);
    if (hm.per_chain) lit_set_chain_mass(lp, sc.dev.mass_diag, hm.t, sc.dev.n_chains);
    else if (hm.shared) { lp.precond = 1; lp.m_sqrt = hm.t.ms.as<double>(); lp.m_inv = hm.t.mi.as<double>(); }
    return launched("hmc (literal replay)", mi::launch_literal(0, lp, rp.n_wg, st));
}

// separable targets (ISO / DIAG), any d, no bounds: no contraction, the elementwise (lane-per-chain) kernels of hmc_diag.hpp
static int run_hmc_elementwise(const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st, const HmcGaussCase& hc)
{
    int rc;
    const uint64_t d = target->d;
    if (hc.dense_m) return fail(MI_ERR_UNSUPPORTED, "hmc: a dense precond_mat is implemented for d <= 128");
    DevBuf prec_owned;
    const double* prec_dev = nullptr;
    if (target->kind == MI_TARGET_GAUSS_DIAG) {
        if (!target->prec) return fail(MI_ERR_BAD_ARG, "GAUSS_DIAG needs prec (d)");
        if (target->mem == MI_MEM_DEVICE) prec_dev = target->prec;
        else {
            HIP_TRY(prec_owned.alloc(d * sizeof(double)));
            HIP_TRY(hipMemcpy(prec_owned.p, target->prec, d * sizeof(double), hipMemcpyHostToDevice));
            prec_dev = prec_owned.as<double>();
        }
    }
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st);
    if (rc) return rc;
    mi::HmcDiagParams q{};
    fill_common(q, d, settings, chains, sc);
    q.prec = prec_dev; q.n_leap = sc.dev.n_leapfrogs;
    q.n_leap_steps = (uint32_t)settings->n_leap_steps; q.eps = settings->step_size;
    WsLease scratch;
    ReplayWs rp = replay_layout(2 * d * chains->n_chains * sizeof(double), chains->n_chains, (uint32_t)d, 0, false, /*needs_matrix=*/false);
    rc = ws_get(st, rp.total_bytes, scratch);
    if (rc) return rc;
    q.scratch = scratch.as<double>();
    rc = replay_bind(rp, scratch.p, chains->n_chains, st);
    if (rc) return rc;
    q.nf_flag = rp.flag;
    int diag_lanes = mi::hmc_diag_pick_lanes(q.C);          // lanes per chain (hmc_diag.hpp)
    if (target->kernel_hint == MI_KERNEL_ELEMENTWISE_1LANE) diag_lanes = 1;
    if (target->kernel_hint == MI_KERNEL_ELEMENTWISE_4LANE) diag_lanes = 4;
    HmcMass hm;
    if ((rc = hmc_mass(hm, q, settings, sc, hc.diag_precond_elementwise, st))) return rc;
    const bool precond = q.m_sqrt != nullptr;        // the PRECOND instantiation: mass tables, per chain or shared
    mi::note_kernel("hmc_diag%d_kernel<%s>", diag_lanes == 4 ? 4 : 1, precond ? "true" : "false");
    if (diag_lanes == 4) hipLaunchKernelGGL(precond ? mi::hmc_diag4_kernel<true> : mi::hmc_diag4_kernel<false>, dim3((unsigned)((q.C + 63) / 64)), dim3(256), 0, st, q);
    else hipLaunchKernelGGL(precond ? mi::hmc_diag1_kernel<true> : mi::hmc_diag1_kernel<false>, dim3((unsigned)((q.C + 255) / 256)), dim3(256), 0, st, q);
    HIP_TRY(hipGetLastError());
    if ((rc = hmc_gauss_replay(target, settings, sc, rp, nullptr, prec_dev, hm, st))) return rc;
    if (hc.diag_precond_elementwise || sc.dev.mass_diag) HIP_TRY(hipStreamSynchronize(st));          // the tables are ours
    return finish(chains, d, settings, sc, st, NO_LEAP_FILL, prec_owned.p != nullptr);
}

// d <= 128, every Gaussian kind: the MFMA tile kernels (hmc_dense.hpp) -- plain, with diagonal masses in the plain kernel's shape, or the general variants
static int run_hmc_tile(const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st, const HmcGaussCase& hc)
{
    int rc;
    const uint64_t d = target->d;
    StagedTarget tg;
    if ((rc = stage_target(target, tg, st))) return rc;
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st);
    if (rc) return rc;

    mi::HmcParams prm{};
    fill_common(prm, d, settings, chains, sc);
    prm.P = tg.mat;
    prm.sep_target = target->kind != MI_TARGET_GAUSS_DENSE;     // ISO / DIAG: the general variants take the gradient element-wise, as the reference's target function does (hmc_dense.hpp: target_times)
    // stream-ordered workspace: P * theta of the last accepted state, [d][C]
    WsLease wsave;
    const size_t d_pad_h = (d <= 16) ? 16 : (d <= 32) ? 32 : (d <= 64) ? 64 : 128;
    ReplayWs rp = replay_layout(3 * d_pad_h * ((chains->n_chains + 15) / 16 + 8) * 16 * sizeof(double), chains->n_chains, (uint32_t)d, 0, false);
    rc = ws_get(st, rp.total_bytes, wsave);
    if (rc) return rc;
    prm.wsave = wsave.as<double>();
    // a diagonal precond_mat alone (no bounds): the plain kernel's shape with two mass tables (hmc_dense.hpp, DIAGM), replay as the plain kernel;
    // per-chain diagonal masses (mi_chains.mass_diag) ride the same variant with [d][C] tables in global memory (PCM)
    const bool chain_mass = sc.dev.mass_diag != nullptr;
    const bool diag_only = (settings->precond_mat != nullptr && !hc.dense_m && !settings->vals_bound) || chain_mass;
    const bool general = hc.bounded && !diag_only;
    if (!general) {                                     // the general variants reproduce the dense products themselves
        rc = replay_bind(rp, wsave.p, chains->n_chains, st);
        if (rc) return rc;
        prm.nf_flag = rp.flag;
    }
    prm.n_leap = sc.dev.n_leapfrogs;
    prm.n_leap_steps = (uint32_t)settings->n_leap_steps;
    prm.eps = settings->step_size;
    prm.stagger = 40;
#ifdef MI_PROFILING     // A/B library only (make prof): the shipped library reads no environment variable
    if (const char* e = getenv("MI_HMC_STAGGER")) prm.stagger = (uint32_t)atoi(e);
    if (const char* e = getenv("MI_HMC_ABLATE")) prm.ablate = (uint32_t)atoi(e);
#endif

    const int nt = (int)((d + 15) / 16);
    if (general) {                                      // bounds and / or a dense precond_mat: the tables of the other samplers' general variants
        GeneralTables gt;
        rc = general_tables("hmc", settings, d, gt, true, true);
        if (rc) return rc;
        prm.btype = gt.bt.as<int>(); prm.lb = gt.lb.as<double>(); prm.ub = gt.ub.as<double>();
        prm.m_sqrt = gt.ms_dev.as<double>(); prm.m_inv = gt.mi_dev.as<double>();
        prm.vals_bound = settings->vals_bound ? 1 : 0;
        if (hc.dense_m) { prm.Minv = gt.minv_full.as<double>(); prm.Lchol = gt.l_full.as<double>(); }
        rc = launched("hmc", mi::launch_hmc_gauss(prm, nt, true, hc.dense_m, st));
        if (!rc) HIP_TRY(hipStreamSynchronize(st));     // the tables are ours
    }
    else {
        // launch shape of the plain kernel (64 < d <= 128): with fewer 16-chain tiles than the chip has wave slots, give a tile
        // a whole SIMD, or two / four of them (hmc_split.hpp).  Estimated cost = rounds of workgroups x time of one round,
        // the round times relative to the two-waves-per-SIMD shape as measured on MI355X.
        int shape = 0;
        if (nt > 4) {
            int dev = 0, n_cu = 256;
            HIP_TRY(hipGetDevice(&dev));
            (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
            if (n_cu <= 0) n_cu = 256;
            const uint64_t C = chains->n_chains;
            auto rounds = [&](uint64_t chains_per_wg) { return (double)(((C + chains_per_wg - 1) / chains_per_wg + n_cu - 1) / n_cu); };
            const double cost[5] = {rounds(128) * 1.00, rounds(64) * MI_HMC_COST_1WAVE, rounds(32) * MI_HMC_COST_SPLIT2,
                                    rounds(32) * MI_HMC_COST_SPLIT4X2, rounds(16) * MI_HMC_COST_SPLIT4};
            for (int k = 1; k < 5; ++k) if (cost[k] < cost[shape]) shape = k;
            switch (target->kernel_hint) {
            case MI_KERNEL_HMC_TWO_WAVES_PER_SIMD: shape = 0; break;
            case MI_KERNEL_HMC_ONE_WAVE_PER_SIMD: shape = 1; break;
            case MI_KERNEL_HMC_SPLIT2: shape = 2; break;
            case MI_KERNEL_HMC_SPLIT4_TWO_WAVES: shape = 3; break;
            case MI_KERNEL_HMC_SPLIT4: shape = 4; break;
            default: break;
            }
        }
        HmcMass hm;
        if ((rc = hmc_mass(hm, prm, settings, sc, diag_only, st))) return rc;
        rc = diag_only  ? launched("hmc", mi::launch_hmc_gauss_diagm(prm, nt, st))
           : shape == 0 ? launched("hmc", mi::launch_hmc_gauss(prm, nt, false, false, st))
                        : launched("hmc", mi::launch_hmc_gauss_few_chains(prm, shape, st));
        if (rc) return rc;
        rc = hmc_gauss_replay(target, settings, sc, rp, tg.mat, nullptr, hm, st);
        if (!rc && diag_only) HIP_TRY(hipStreamSynchronize(st));     // the tables are ours
    }
    if (rc) return rc;
    return finish(chains, d, settings, sc, st, NO_LEAP_FILL, tg.owns());      // (a staged target / host-mode chains must outlive the kernel)
}
}  // namespace

int mi_mcmc_hmc_run(const mi_target* target, const mi_settings* settings, mi_chains* chains, void* stream)
{
    int rc = check_common(target, settings, chains, true);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t d = target->d;
    if (chains->mass_diag) {
        // per-chain diagonal masses: separable Gaussians without bounds on the elementwise kernels (below), everything else literally
        const bool sep = target->kind == MI_TARGET_GAUSS_ISO || target->kind == MI_TARGET_GAUSS_DIAG;
        // ... a dense precision with d <= 128, no bounds: the MFMA kernel with per-chain tables (round 4; the literal kernel served it before)
        const bool dense_mfma = target->kind == MI_TARGET_GAUSS_DENSE && d <= 128 && !settings->vals_bound;
        if ((!sep && !dense_mfma) || settings->vals_bound) {
            if (target->kind == MI_TARGET_NORMAL_MODEL) return fail(MI_ERR_UNSUPPORTED, "hmc: chains.mass_diag with the normal-model target is not implemented");
            return run_literal("hmc", 0, target, settings, chains, st);
        }
    }
    if (target->kind == MI_TARGET_NORMAL_MODEL) return run_small_normal_model("hmc", 0, target, settings, chains, st);
    if (target->kind == MI_TARGET_LOGISTIC && gemm_case(target, settings, chains, true, true, st)) return run_gemm("hmc", 0, target, settings, chains, st);   // d > 512, plain: two matrix products per leapfrog step
    if (target->kind == MI_TARGET_LOGISTIC) {      // plain: the LDS-staged MFMA kernel (d <= 512); bounds / precond_mat: one chain per lane (d <= 8); else literal.hpp
        // a DIAGONAL precond_mat alone rides the LDS-staged kernel too (its DIAGM instantiation: two tables read from global memory)
        // ... and so do bounds (its BOUNDS instantiation, lds_box.hpp), with the identity or a diagonal matrix
        // ... and, round 5, a DENSE precond_mat without bounds (DENSEM: INV(M) and CHOL_LOWER(M) streamed through LDS like X)
        const bool lds_general = (settings->vals_bound || settings->precond_mat) && (lds_general_ok(target, settings) || lds_dense_m_ok(target, settings))
                                 && d > (uint64_t)mi::SMALL_MAX_D && d <= 512;
        if ((settings->vals_bound || settings->precond_mat) && !lds_general)
            return d <= (uint64_t)mi::SMALL_MAX_D ? run_small_logistic("hmc", 0, target, settings, chains, st) : run_literal("hmc", 0, target, settings, chains, st);
        return d <= 512 ? run_lds("hmc", mi::LOGIT_HMC, target, settings, chains, st, mi::LOGIT_TARGET_LOGISTIC) : run_literal("hmc", 0, target, settings, chains, st);
    }
    if (target->kind != MI_TARGET_GAUSS_ISO && target->kind != MI_TARGET_GAUSS_DIAG && target->kind != MI_TARGET_GAUSS_DENSE)
        return fail(MI_ERR_UNSUPPORTED, "hmc: target kind %d not implemented", target->kind);
    // precond_mat (hmc.cpp:57-59): INV and CHOL_LOWER of a DIAGONAL matrix are the element-wise 1/m and sqrt(m), exactly what the oracle's
    // Gauss-Jordan / Cholesky produce; a dense matrix: three fragment sets in LDS (d <= 64), or the two extra ones read from L2 in fragment
    // order (64 < d <= 128) -- the tables come from settings_host.hpp where a route below needs them
    const bool dense_m = mi::settings::precond_kind(settings->precond_mat, d) == 2;
    // beyond d = 128 the tiled kernels serve separable targets without bounds (identity or diagonal precond_mat: hmc_diag.hpp);
    // everything else there -- dense gradients, bounds, a dense precond_mat -- runs on the literal kernel (literal.hpp)
    if (d > 128 && d <= 512 && target->kind == MI_TARGET_GAUSS_DENSE && !(dense_m && settings->vals_bound) && target->kernel_hint != MI_KERNEL_LITERAL)
        return run_lds("hmc", mi::LOGIT_HMC, target, settings, chains, st, mi::LOGIT_TARGET_DENSE);      // P streamed through LDS (logistic_lds.hpp); identity or diagonal precond_mat, with or without bounds; a dense one without
    if (gemm_case(target, settings, chains, true, true, st)) return run_gemm("hmc", 0, target, settings, chains, st);      // one matrix product per leapfrog step (gemm_samplers.hip)
    if (d > 128 && (target->kind == MI_TARGET_GAUSS_DENSE || settings->vals_bound || dense_m))
        return run_literal("hmc", 0, target, settings, chains, st);
    const bool bounded = settings->vals_bound != 0 || settings->precond_mat != nullptr;   // the general kernel variant
    if (settings->vals_bound && (!settings->lower_bounds || !settings->upper_bounds))
        return fail(MI_ERR_BAD_ARG, "hmc: vals_bound needs lower_bounds and upper_bounds");
    const bool separable_kind = target->kind == MI_TARGET_GAUSS_ISO || target->kind == MI_TARGET_GAUSS_DIAG;
    // separable target + diagonal precond_mat (no bounds): the elementwise kernel, any d
    const bool diag_precond_elementwise = separable_kind && !settings->vals_bound && settings->precond_mat && !dense_m && d > 128;
    if (bounded && d > 128 && !diag_precond_elementwise) return fail(MI_ERR_UNSUPPORTED, "hmc: vals_bound with d > 128 is not implemented");
    if (settings->n_burnin_draws + settings->n_keep_draws > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "too many draws");
    const bool separable = target->kind != MI_TARGET_GAUSS_DENSE;
    // kernel_hint (mi_mcmc.h): an explicit request for the elementwise kernels where the MFMA kernel would be picked; every
    // kernel produces the same bits, so the hint changes speed only
    const bool force_diag = !bounded && (target->kernel_hint == MI_KERNEL_ELEMENTWISE_1LANE || target->kernel_hint == MI_KERNEL_ELEMENTWISE_4LANE);
    if (d > 128 && !separable)
        return fail(MI_ERR_UNSUPPORTED, "hmc: d = %llu > 128 not implemented for dense-gradient targets", (unsigned long long)d);
    const HmcGaussCase hc{dense_m, bounded, diag_precond_elementwise};
    if (separable && (d > 128 || force_diag || chains->mass_diag)) return run_hmc_elementwise(target, settings, chains, st, hc);
    return run_hmc_tile(target, settings, chains, st, hc);
}

int mi_mcmc_rmhmc_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel, void* target_data,
                               mi_tensor_cb tensor_fn, void* tensor_data, const mi_settings* settings, double* draws_out,
                               uint64_t* n_accept_draws)
{
    if (!tensor_fn) return fail(MI_ERR_BAD_ARG, "rmhmc (callback): null tensor_fn");
    return mi::host::literal_run_callback("rmhmc", 4, initial_vals, d, target_log_kernel, target_data, tensor_fn, tensor_data, settings, draws_out,
                                          n_accept_draws, nullptr);
}

namespace {
// mala on the Gaussian kinds with d <= 128: the MFMA tile kernels (mala_dense.hpp) -- plain, general (bounds and / or a diagonal precond_mat), a dense precond_mat
// without bounds; with both the literal kernel runs the call entirely
static int run_mala_tile(const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st)
{
    int rc;
    const uint64_t d = target->d;
    StagedTarget tg;
    if ((rc = stage_target(target, tg, st))) return rc;
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st);
    if (rc) return rc;

    mi::MalaParams prm{};
    fill_common(prm, d, settings, chains, sc);
    prm.P = tg.mat;
    prm.eps = settings->step_size;
    // Sigma = eps^2 * I (mala.ipp:41,63): INV by Gauss-Jordan gives diag(1/s2); CHOL gives diag(sqrt(s2));
    // LOG_DET = sum_i 2 log L_ii accumulated sequentially, exactly as the oracle states it (settings_host.hpp: mala_sigma).
    mi::settings::MalaSigma sg;
    (void)mi::settings::mala_sigma(d, settings->step_size, 0, nullptr, sg);
    prm.s2 = settings->step_size * settings->step_size; prm.rs = sg.rs; prm.cons_term = sg.cons_term; prm.log_det = sg.log_det;

    const int nt = (int)((d + 15) / 16);
    GeneralTables gt;
    rc = general_tables("mala", settings, d, gt, true, true);
    if (rc) return rc;
    // literal replay (literal.hpp): the chains the element-wise kernels flag as non-finite; bounded mala with a dense precond_mat
    // (INV(eps^2 J(theta') M) per draw, mala.ipp:52-53) runs there entirely
    const bool mala_bounded = settings->vals_bound != 0;
    const bool literal_only = gt.active && gt.dense && mala_bounded;
    const bool dense_unbounded = gt.active && gt.dense && !mala_bounded;   // real dense products (sep_target: element-wise where the reference is): nothing to replay
    WsLease lws;
    ReplayWs rp = replay_layout(0, chains->n_chains, (uint32_t)d, 0, mala_bounded);
    mi::lit::LitParams lp{};
    LitDev ldev;
    if (!dense_unbounded) {
        rc = ws_get(st, rp.total_bytes, lws);
        if (rc) return rc;
        rc = replay_bind(rp, lws.p, chains->n_chains, st);
        if (rc) return rc;
        rc = lit_gauss_target(lp.t, target->kind, (uint32_t)d, tg.mat, nullptr, rp.tbuf, st);
        if (rc) return rc;
        lit_common(lp, settings, &sc.dev, rp, literal_only);
        mi::lit::LitPrep prep;
        rc = mi::lit::lit_prepare(1, (uint32_t)d, settings->step_size, settings->vals_bound ? 1 : 0, settings->lower_bounds,
                                  settings->upper_bounds, settings->precond_mat, prep);
        if (rc) return rc;
        rc = lit_upload(prep, (uint32_t)d, mala_bounded, ldev, lp);
        if (rc) return rc;
        prm.nf_flag = rp.flag;
    }
    if (literal_only) {
        rc = launched("mala (literal)", mi::launch_literal(1, lp, rp.n_wg, st));
    }
    else if (dense_unbounded) {
        // dense precond_mat, unbounded: Sigma = eps^2 M is constant, so INV / CHOL_LOWER / LOG_DET come from the host once
        rc = mi::settings::mala_sigma(d, settings->step_size, 2, settings->precond_mat, sg); if (rc) return rc;
        prm.log_det = sg.log_det;
        DevBuf m_full, sinv_full;
        rc = upload_matrix(std::vector<double>(settings->precond_mat, settings->precond_mat + d * d), d, m_full); if (rc) return rc;
        rc = upload_matrix(sg.Sinv, d, sinv_full); if (rc) return rc;
        prm.Mfull = m_full.as<double>(); prm.Lchol = gt.l_full.as<double>(); prm.Sinv = sinv_full.as<double>();
        prm.sep_target = target->kind != MI_TARGET_GAUSS_DENSE;     // ISO / DIAG: the gradient is element-wise in the reference's target function
        rc = launched("mala", mi::launch_mala_gauss(prm, nt, 2, st));
        if (!rc) HIP_TRY(hipStreamSynchronize(st));     // the matrices are ours
    }
    else if (gt.active) {
        // unbounded runs hoist LOG_DET(eps^2 M) = sum_i 2 log sqrt(eps^2 M_ii), i ascending (bounded runs sum it per draw)
        (void)mi::settings::mala_sigma(d, settings->step_size, 1, gt.m.data(), sg);
        prm.log_det = sg.log_det;
        if ((rc = gt.upload_m())) return rc;
        prm.vals_bound = settings->vals_bound ? 1 : 0;
        prm.btype = gt.bt.as<int>(); prm.lb = gt.lb.as<double>(); prm.ub = gt.ub.as<double>();
        prm.m = gt.m_dev.as<double>(); prm.m_sqrt = gt.ms_dev.as<double>();
        rc = launched("mala", mi::launch_mala_gauss(prm, nt, 1, st));
        if (!rc) rc = launched("mala (literal replay)", mi::launch_literal(1, lp, rp.n_wg, st));
    }
    else {
        rc = launched("mala", mi::launch_mala_gauss(prm, nt, 0, st));
        if (!rc) rc = launched("mala (literal replay)", mi::launch_literal(1, lp, rp.n_wg, st));
    }
    if (rc) return rc;
    if (gt.active || ldev.any) HIP_TRY(hipStreamSynchronize(st));     // the tables are ours
    return finish(chains, d, settings, sc, st, 0, tg.owns());
}
}  // namespace

int mi_mcmc_mala_run(const mi_target* target, const mi_settings* settings, mi_chains* chains, void* stream)
{
    int rc = check_common(target, settings, chains);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t d = target->d;
    if (settings->n_burnin_draws + settings->n_keep_draws > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "too many draws");
    if (target->kind == MI_TARGET_NORMAL_MODEL) return run_small_normal_model("mala", 1, target, settings, chains, st);
    // a DIAGONAL precond_mat alone rides the LDS-staged kernel too (its DIAGM instantiation)
    // ... and, round 5, a DENSE one without bounds (DENSEM: M, CHOL_LOWER(M) and INV(eps^2 M) streamed through LDS like X)
    const bool mala_diag_alone = !settings->vals_bound && (precond_is_diagonal(settings, d) || lds_dense_m_ok(target, settings)) && d > (uint64_t)mi::SMALL_MAX_D && d <= 512;
    if (target->kind == MI_TARGET_LOGISTIC && gemm_case(target, settings, chains, false, true, st)) return run_gemm("mala", 1, target, settings, chains, st);    // d > 512, identity or a diagonal precond_mat, no bounds
    if (target->kind == MI_TARGET_LOGISTIC && (settings->vals_bound || settings->precond_mat) && !mala_diag_alone)
        return d <= (uint64_t)mi::SMALL_MAX_D ? run_small_logistic("mala", 1, target, settings, chains, st) : run_literal("mala", 1, target, settings, chains, st);
    if (target->kind == MI_TARGET_LOGISTIC && d > 512) return run_literal("mala", 1, target, settings, chains, st);
    if (target->kind == MI_TARGET_LOGISTIC) return run_lds("mala", mi::LOGIT_MALA, target, settings, chains, st, mi::LOGIT_TARGET_LOGISTIC);
    if (target->kind != MI_TARGET_GAUSS_ISO && target->kind != MI_TARGET_GAUSS_DIAG && target->kind != MI_TARGET_GAUSS_DENSE)
        return fail(MI_ERR_UNSUPPORTED, "mala: target kind %d not implemented", target->kind);
    if (d > 128 && d <= 512 && target->kind == MI_TARGET_GAUSS_DENSE && !settings->vals_bound
        && (!settings->precond_mat || precond_is_diagonal(settings, d) || lds_dense_m_ok(target, settings)))
        return run_lds("mala", mi::LOGIT_MALA, target, settings, chains, st, mi::LOGIT_TARGET_DENSE);     // P streamed through LDS (logistic_lds.hpp); identity, diagonal or (round 5) dense precond_mat
    if (gemm_case(target, settings, chains, false, true, st)) return run_gemm("mala", 1, target, settings, chains, st);    // one matrix product per draw (gemm_samplers.hip)
    if (d > 128) return run_literal("mala", 1, target, settings, chains, st);      // no other tiled kernel beyond d = 128: literal.hpp
    return run_mala_tile(target, settings, chains, st);
}

namespace {
// rwmh on the Gaussian kinds with d <= 128: the MFMA tile kernels (rwmh_dense.hpp), plain or general (bounds and / or a cov_mat)
static int run_rwmh_tile(const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st)
{
    int rc;
    const uint64_t d = target->d;
    StagedTarget tg;
    if ((rc = stage_target(target, tg, st))) return rc;
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st);
    if (rc) return rc;

    mi::RwmhParams prm{};
    fill_common(prm, d, settings, chains, sc);
    prm.P = tg.mat;
    prm.par_scale = settings->step_size;

    const int nt = (int)((d + 15) / 16);
    GeneralTables gt;
    rc = general_tables("rwmh", settings, d, gt, true, true);
    if (rc) return rc;
    DevBuf c_dev, lc_dev;
    if (gt.active) {
        // cov_mcmc_chol = par_scale * CHOL_LOWER(cov_mat), element by element (rwmh.cpp:119)
        std::vector<double> c(d);
        for (uint64_t i = 0; i < d; ++i) c[i] = prm.par_scale * gt.m_sqrt[i];
        HIP_TRY(c_dev.alloc(d * 8));
        HIP_TRY(hipMemcpy(c_dev.p, c.data(), d * 8, hipMemcpyHostToDevice));
        prm.vals_bound = settings->vals_bound ? 1 : 0;
        prm.btype = gt.bt.as<int>(); prm.lb = gt.lb.as<double>(); prm.ub = gt.ub.as<double>();
        prm.c_diag = c_dev.as<double>();
        if (gt.dense) {
            std::vector<double> L = gt.L;
            for (auto& v : L) v = prm.par_scale * v;
            rc = upload_matrix(L, d, lc_dev); if (rc) return rc;
            prm.Lc = lc_dev.as<double>();
        }
        rc = launched("rwmh", mi::launch_rwmh_gauss(prm, nt, true, gt.dense, st));
        if (!rc) HIP_TRY(hipStreamSynchronize(st));     // the tables are ours
    }
    else rc = launched("rwmh", mi::launch_rwmh_gauss(prm, nt, false, false, st));
    if (rc) return rc;
    return finish(chains, d, settings, sc, st, 0, tg.owns());
}
}  // namespace

// mcmc::rwmh (src/rwmh.cpp:30-175) for many chains.  settings->step_size carries rwmh_settings.par_scale and
// settings->precond_mat carries rwmh_settings.cov_mat (identity when NULL, rwmh.cpp:58).
int mi_mcmc_rwmh_run(const mi_target* target, const mi_settings* settings, mi_chains* chains, void* stream)
{
    int rc = check_common(target, settings, chains);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t d = target->d;
    if (target->kind == MI_TARGET_NORMAL_MODEL) return run_small_normal_model("rwmh", 3, target, settings, chains, st);
    if (target->kind == MI_TARGET_LOGISTIC && gemm_case(target, settings, chains, false, false, st)) return run_gemm("rwmh", 3, target, settings, chains, st);    // d > 512, plain or with bounds
    if (target->kind == MI_TARGET_LOGISTIC) {
        if (settings->vals_bound || settings->precond_mat)
            return d <= (uint64_t)mi::SMALL_MAX_D ? run_small_logistic("rwmh", 3, target, settings, chains, st) : run_literal("rwmh", 3, target, settings, chains, st);
        return d <= 512 ? run_lds("rwmh", mi::LOGIT_RWMH, target, settings, chains, st, mi::LOGIT_TARGET_LOGISTIC) : run_literal("rwmh", 3, target, settings, chains, st);
    }
    if (target->kind != MI_TARGET_GAUSS_ISO && target->kind != MI_TARGET_GAUSS_DIAG && target->kind != MI_TARGET_GAUSS_DENSE)
        return fail(MI_ERR_UNSUPPORTED, "rwmh: target kind %d not implemented", target->kind);
    if (d > 128 && d <= 512 && target->kind == MI_TARGET_GAUSS_DENSE && !settings->vals_bound && !settings->precond_mat)
        return run_lds("rwmh", mi::LOGIT_RWMH, target, settings, chains, st, mi::LOGIT_TARGET_DENSE);     // P streamed through LDS (logistic_lds.hpp)
    if (gemm_case(target, settings, chains, false, false, st)) return run_gemm("rwmh", 3, target, settings, chains, st);
    if (d > 128) return run_literal("rwmh", 3, target, settings, chains, st);      // no other tiled kernel beyond d = 128: literal.hpp
    return run_rwmh_tile(target, settings, chains, st);
}

// nuts on the LDS-streamed evaluation (nuts_lds.hpp): the logistic target with 8 < d <= 512 and dense Gaussians with 128 < d <= 512,
// identity precond_mat, no bounds, 1 <= max_tree_depth <= 10.  Chains that reach the non-finite regime are flagged by the kernel and
// replayed by literal_kernel<2> right behind it.  lds_target: mi::LOGIT_TARGET_LOGISTIC / mi::LOGIT_TARGET_DENSE.
int run_lds_nuts(const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st, int lds_target)
{
    int rc;
    const uint64_t d = target->d, C = chains->n_chains;
    const uint64_t n_total = settings->n_burnin_draws + settings->n_keep_draws;
    if (n_total > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "too many draws");
    const bool dense = lds_target == mi::LOGIT_TARGET_DENSE;
    StagedTarget tg;
    if ((rc = stage_target(target, tg, st))) return rc;
    const uint64_t n_rows = tg.n_rows;
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st, n_total);
    if (rc) return rc;
    mi::LogitParams q{};
    fill_common(q, d, settings, chains, sc);
    q.n_rows = (uint32_t)n_rows; q.NB = (uint32_t)((n_rows + 15) / 16);
    q.n_leap_out = sc.dev.n_leapfrogs;
    q.n_exec_out = sc.dev.n_leapfrogs_executed; sc.exec_written = q.n_exec_out != nullptr;      // (every doubling on a memoised trajectory: nuts_lds.hpp)
    if ((rc = fill_nuts(q, settings, chains, sc))) return rc;
    q.eps_bar0 = settings->step_size;
    // a DENSE precond_mat without bounds (round 6): INV(M) and CHOL_LOWER(M) streamed through LDS like the target's matrix (nuts_lds.hpp: DENSEM)
    const bool dense_m = lds_dense_m_ok(target, settings);
    LdsTables lt;
    LdsDenseM ldm;
    if (dense_m) { if ((rc = lds_dense_m(settings, d, ldm, q, mi::LOGIT_HMC))) return rc; }
    else if ((rc = lds_tables("nuts", settings, d, lt, q))) return rc;      // (the caller routed bounds / a DIAGONAL matrix here)

    // workspace: the kernel's own | non-finite flags | the matrix transposed and the work areas of the literal replay
    ReplayWs rp;
    rp.t_doubles = ((size_t)d * std::max<size_t>(d, n_rows) + 31) & ~(size_t)31;
    // (the kernel's workspace is sized by the chain SLOTS of its persistent grid, not by the chains)
    const uint64_t n_slots = 32 * (dense_m ? mi::logit_lds_nuts_dense_m_workgroups(q.d, C, lds_target) : mi::logit_lds_nuts_workgroups(q.d, C, lds_target));
    rp.own_bytes = (mi::logit_lds_workspace_bytes(q.d, q.NB, n_slots, lds_target, mi::LOGIT_NUTS) + 255) & ~(size_t)255;
    rp.stride = mi::lit::lit_work_doubles((uint32_t)d, dense ? 0u : (uint32_t)n_rows, false, q.max_depth, true, false);
    rp.n_wg = (unsigned)std::min<uint64_t>(C, 512u);
    const size_t flag_bytes = ((C + 1) * sizeof(uint32_t) + 255) & ~(size_t)255;
    rp.total_bytes = rp.own_bytes + flag_bytes + (rp.t_doubles + (size_t)rp.n_wg * rp.stride) * sizeof(double);
    // more chains than chain slots: the launcher cuts the runs into pieces (lds_nuts_pieces.hpp) and needs room for the queues
    const size_t rp_bytes = (rp.total_bytes + 255) & ~(size_t)255;
    const size_t split_bytes = (C > n_slots) ? mi::logit_lds_nuts_split_bytes(C, q.d) : 0;
    WsLease base;
    rc = ws_get(st, rp_bytes + split_bytes, base);
    if (rc) return rc;
    rc = replay_bind(rp, base.p, C, st);
    if (rc) return rc;
    q.nf_flag = rp.flag;
    if (split_bytes) q.split_ws = static_cast<char*>(base.p) + rp_bytes;
    DevBuf mws;                                          // dense_m: the block images of the two matrices (+ the exchange vectors of their products)
    if (dense_m) HIP_TRY(mws.alloc(mi::logit_lds_nuts_dense_m_bytes(q.d, C, lds_target)));
    const int e = dense_m ? mi::logit_lds_launch_nuts_dense_m(q, tg.mat, tg.y, base.p, mws.p, st, lds_target)
                          : mi::logit_lds_launch(mi::LOGIT_NUTS, q, tg.mat, tg.y, base.p, st, lds_target);
    if (e != 0) return fail(MI_ERR_HIP, "LDS-streamed nuts kernel launch: %s", hipGetErrorString((hipError_t)e));
    const std::string lds_name = mi::host::last_kernel();
    {
        mi::lit::LitParams lp{};
        if ((rc = lit_staged_target(lp.t, tg, (uint32_t)d, rp.tbuf, st))) return rc;
        lit_common(lp, settings, &sc.dev, rp, false);
        if ((rc = fill_nuts(lp, settings, chains, sc))) return rc;
        LitDev ldev;
        if (dense_m) {                                   // the replay's own copies of M, INV(M), CHOL_LOWER(M) (transposed: literal_host.hpp)
            mi::lit::LitPrep prep;
            rc = mi::lit::lit_prepare(0, (uint32_t)d, settings->step_size, 0, nullptr, nullptr, settings->precond_mat, prep);
            if (rc) return rc;
            rc = lit_upload(prep, (uint32_t)d, false, ldev, lp);
            if (rc) return rc;
        }
        else lds_tables_replay(lt, q, lp);
        rc = launched("LDS-streamed nuts kernel (literal replay)", mi::launch_literal(2, lp, rp.n_wg, st));
        if (!rc && q.n_exec_out) rc = copy_flagged_counts(rp.flag, q.n_leap_out, q.n_exec_out, C, st);      // a replayed chain executed every leapfrog it counts
        if (!rc && dense_m) HIP_TRY(hipStreamSynchronize(st));     // (the replay's matrices are ours)
        if (rc) return rc;
        mi::host::last_kernel() = lds_name;
    }
    return finish(chains, d, settings, sc, st, NO_LEAP_FILL, tg.owns() || lt.ms.p || dense_m, n_total);
}
// the cases nuts_lds.hpp covers (everything else on these targets: literal.hpp): no bounds / bounds with the identity or a diagonal precond_mat, and --
// round 6 -- a DENSE precond_mat without bounds
bool lds_nuts_case(const mi_target* target, const mi_settings* settings)
{
    return (lds_general_ok(target, settings) || lds_dense_m_ok(target, settings)) && settings->max_tree_depth >= 1 && settings->max_tree_depth <= 10;
}

// The plain case (unbounded; identity or a diagonal precond_mat) runs on nuts_memo.hpp.  The register-carried kernels of rounds 2-4 (nuts_reg.hpp,
// nuts_dyn.hpp, nuts_split.hpp) are retired: the memoised kernel is faster wherever a leapfrog costs anything (d = 128: 563 ms against 699 at
// 65 536 chains, 135 / 156 at 8 192; d = 64: 209 / 208; d = 32: 71 / 72) and within 13 % at d = 16 (37 / 33 ms) -- one tick to maintain instead of
// four.  Their hints stay valid and are ignored.  MI_KERNEL_NUTS_TICK_LOCAL keeps the independent tick-local kernel for A/B runs.

// nuts on the matrix-product route (gemm_nuts.hpp): the dense Gaussian and the logistic target BEYOND d = 512, identity or a DIAGONAL precond_mat, with or without
// vals_bound, 1 <= max_tree_depth <= 10 -- per-chain memoised trees, one product per tick for all chains.  Capacity is a routing condition, then chunking: a chain holds
// gemm_nuts_chain_bytes of workspace (0.85 MB at d = 1024, max_tree_depth 10; with bounds one vector of padded d more), so a call whose chains do not fit the free device memory (plus this stream's cached
// workspace) together runs them as consecutive RANGES, in multiples of 128, through the same code -- chains are independent and their random numbers are
// counter-based on the global chain index, so the bits do not change -- and a call for which not even one range of 128 fits stays on the literal kernel.
struct GemmNutsPlan { uint64_t range = 0; size_t own_bytes = 0; };
constexpr uint64_t GEMM_NUTS_BOUNDED_MIN_CHAINS = 16;
bool gemm_nuts_case(const mi_target* target, const mi_settings* settings, const mi_chains* chains, hipStream_t st, GemmNutsPlan& plan)
{
    if (!((target->kind == MI_TARGET_GAUSS_DENSE || target->kind == MI_TARGET_LOGISTIC) && target->d > 512 && target->kernel_hint != MI_KERNEL_LITERAL)) return false;
    if (chains->mass_diag || settings->max_tree_depth < 1 || settings->max_tree_depth > 10) return false;
    if (settings->precond_mat && !precond_is_diagonal(settings, target->d)) return false;
    const uint64_t d = target->d, C = chains->n_chains, n = target->kind == MI_TARGET_LOGISTIC ? target->n_rows : 0;
    if (d > 131056ULL || n > 0x7fffffffULL) return false;                                   // (grid.y of the element-wise kernel: padded d / 2)
    const uint32_t D = (uint32_t)settings->max_tree_depth;
    const bool bounded = settings->vals_bound != 0;      // (missing bound arrays: run_gemm_nuts reports them.  The replay's work areas do not grow with bounds: `rest` below)
    // A bounded call of fewer than 16 chains -- less than one wave of the per-chain kernel (16 chains x 4 lanes) -- stays on the literal kernel, as before: the routing
    // tests of the suite hold such calls there (6 chains), and the route was measured from 128 chains up only.  Not a measured crossover
    if (bounded && C < GEMM_NUTS_BOUNDED_MIN_CHAINS) return false;
    const size_t chain_b = mi::gemm::gemm_nuts_chain_bytes((uint32_t)d, (uint32_t)n, D, bounded), fixed_b = mi::gemm::gemm_nuts_fixed_bytes((uint32_t)d, (uint32_t)n);
    size_t budget = (size_t)g_gemm_nuts_ws_bytes.load(std::memory_order_relaxed);           // (the test hook: the route's own workspace, as if this were all there is)
    if (budget == 0) {
        // next to the route's own: the flags and the literal replay's matrix and work areas, a host target's matrix and the tables
        const size_t rest = (C + 1) * sizeof(uint32_t) + ((size_t)d * std::max<size_t>(d, n) + 64 + (size_t)std::min<uint64_t>(C, 512u)
                            * mi::lit::lit_work_doubles((uint32_t)d, (uint32_t)n, false, D, true, false)) * sizeof(double) + (size_t)d * std::max<size_t>(d, n) * sizeof(double) + ((size_t)1 << 20);
        // ... and what stage_in allocates for chains in host memory, for the whole call whatever the ranges: theta, draws, nuts_depth, the per-chain arrays; the labels of a host target
        size_t staged = 0;
        if (chains->mem == MI_MEM_HOST) {
            const size_t n_tot = (size_t)(settings->n_burnin_draws + settings->n_keep_draws);
            staged = (size_t)d * C * sizeof(double) + (chains->draws ? (size_t)settings->n_keep_draws * d * C * sizeof(double) : 0)
                     + (chains->nuts_depth ? n_tot * C * sizeof(uint32_t) : 0)
                     + 8 * C * sizeof(double);           // stage_in's per-chain arrays: n_accept, step_size, n_leapfrogs, n_leapfrogs_executed, nuts_adapt_state [3] (7 C words; one spare)
        }
        if (target->mem == MI_MEM_HOST) staged += (size_t)n * sizeof(double);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
        const size_t have = free_b + ws_cached_bytes(st);      // (the cached workspace of this stream is given back before a larger one is taken)
        budget = have > rest + staged ? have - rest - staged : 0;
    }
    uint64_t range = mi::gemm::gemm_nuts_range_chains(C, chain_b, fixed_b, budget);
    range = std::min<uint64_t>(range, (uint64_t)65535 * 64 / 128 * 128);                     // (grid.x of the class-wise kernel: padded chains / 64)
    if (range < 128) return false;
    plan.range = range;
    plan.own_bytes = fixed_b + (size_t)range * chain_b;
    return true;
}
int run_gemm_nuts(const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st, const GemmNutsPlan& plan)
{
    int rc;
    const uint64_t d = target->d, C = chains->n_chains;
    const bool logit = target->kind == MI_TARGET_LOGISTIC;
    const uint64_t n = logit ? target->n_rows : 0;
    const uint64_t n_total = settings->n_burnin_draws + settings->n_keep_draws;
    if (n_total > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "too many draws");
    const bool bounded = settings->vals_bound != 0;
    if (bounded && (!settings->lower_bounds || !settings->upper_bounds)) return fail(MI_ERR_BAD_ARG, "nuts: vals_bound needs lower_bounds and upper_bounds");
    StagedTarget tg;
    if ((rc = stage_target(target, tg, st))) return rc;
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st, n_total);
    if (rc) return rc;
    mi::gemm::GemmNutsRun g;
    fill_common(g, d, settings, chains, sc);             // (g.C: the range loop below sets it per range)
    g.C_total = C; g.n_rows = (uint32_t)n;
    if (logit) { g.X = tg.mat; g.y = tg.y; } else g.P = tg.mat;
    g.n_leap = sc.dev.n_leapfrogs; g.n_exec = sc.dev.n_leapfrogs_executed;
    g.step = sc.dev.step_size; g.depth = sc.dev.nuts_depth; g.adapt = sc.dev.nuts_adapt_state;
    sc.exec_written = g.n_exec != nullptr;               // (every doubling on a memoised trajectory)
    if ((rc = fill_nuts_adapt(g, settings, chains))) return rc;
    g.eps_bar0 = settings->step_size;
    // identity or a DIAGONAL precond_mat: diag(M), CHOL_LOWER (sqrt), INV (reciprocal) from lit_prepare, in the oracle's operation order; the identity as tables of ones
    mi::lit::LitPrep prep;
    // (and, vals_bound, the bounds tables of the same derivation: what bounded hmc on this route reads)
    rc = mi::lit::lit_prepare(0, (uint32_t)d, settings->step_size, bounded ? 1 : 0, settings->lower_bounds, settings->upper_bounds, settings->precond_mat, prep);
    if (rc) return rc;
    const uint32_t dK = mi::gemm::gemm_padded_d((uint32_t)d);
    GemmBoxTables box;
    if (bounded) {
        if ((rc = gemm_box_tables(prep, d, dK, box))) return rc;
        g.bounded = true; g.btype = box.btype; g.lb = box.lb; g.ub = box.ub; g.box_blocks = box.blocks;
    }
    std::vector<double> tabs;
    gemm_mass_tables(prep, d, dK, 3, tabs);
    DevBuf tabs_dev;
    if ((rc = upload_padded(tabs_dev, tabs.data(), tabs.size(), tabs.size(), 1.0))) return rc;
    g.mass_tables = tabs_dev.as<double>(); g.diag_mass = prep.precond == 1;
    // workspace: the route's own (the packed matrices, one range of chains) | non-finite flags | the matrix transposed and the work areas of the literal replay
    ReplayWs rp;
    rp.t_doubles = ((size_t)d * std::max<size_t>(d, n) + 31) & ~(size_t)31;
    rp.own_bytes = (plan.own_bytes + 255) & ~(size_t)255;
    rp.stride = mi::lit::lit_work_doubles((uint32_t)d, (uint32_t)n, false, g.max_depth, true, false);
    rp.n_wg = (unsigned)std::min<uint64_t>(C, 512u);
    const size_t flag_bytes = ((C + 1) * sizeof(uint32_t) + 255) & ~(size_t)255;
    rp.total_bytes = rp.own_bytes + flag_bytes + (rp.t_doubles + (size_t)rp.n_wg * rp.stride) * sizeof(double);
    WsLease base;
    rc = ws_get(st, rp.total_bytes, base);
    if (rc) return rc;
    rc = replay_bind(rp, base.p, C, st);
    if (rc) return rc;
    g.nf_flag = rp.flag;
    g.ws = base.p;
    const char* kname = nullptr;
    uint64_t ticks = 0, points = 0, slots = 0;
    const bool may_graph = g_gemm_graph_mode.load(std::memory_order_relaxed) == 0;      // (the test hook: never capture)
    for (uint64_t c_off = 0; c_off < C; c_off += plan.range) {           // the chains as consecutive ranges: the same code, the global chain index
        g.c_off = c_off; g.C = std::min<uint64_t>(plan.range, C - c_off); g.pack = c_off == 0;
        // a tick is a handful of short launches while the chains are few: replayed from a captured (linear) graph; at full size the queue runs ahead anyway
        // (the threshold is run_gemm's, taken over and not varied here: at d = 1024 the measured tick is far longer than a launch on both sides of it -- DESIGN 4.22)
        g.use_graph = may_graph && (double)d * (double)(logit ? 2 * n : d) * (double)g.C < 3.0e10;
        const int e = mi::gemm::gemm_nuts_run(g, st, &kname);
        if (e != 0) return fail(MI_ERR_HIP, "nuts: matrix-product sampler: %s", hipGetErrorString((hipError_t)e));
        if (g.still_running != 0)
            return fail(MI_ERR_HIP, "nuts: matrix-product sampler: %llu chains still running after the ceiling of %llu ticks", (unsigned long long)g.still_running, (unsigned long long)g.ticks_run);
        g_gemm_nuts_ranges.fetch_add(1, std::memory_order_relaxed);
        ticks += g.ticks_run; points += g.points_taken; slots += g.ticks_run * g.C;
    }
    g_gemm_nuts_ticks.store(ticks, std::memory_order_relaxed); g_gemm_nuts_points.store(points, std::memory_order_relaxed); g_gemm_nuts_slots.store(slots, std::memory_order_relaxed);
    {   // chains that reached the non-finite regime (or ran past the search's allowance): replayed literally (literal.hpp)
        mi::lit::LitParams lp{};
        if ((rc = lit_staged_target(lp.t, tg, (uint32_t)d, rp.tbuf, st))) return rc;
        lit_common(lp, settings, &sc.dev, rp, false);
        if ((rc = fill_nuts(lp, settings, chains, sc))) return rc;
        if (prep.precond == 1) { lp.precond = 1; lp.m = g.mass_tables; lp.m_sqrt = g.mass_tables + dK; lp.m_inv = g.mass_tables + 2 * (size_t)dK; }
        if (bounded) { lp.vals_bound = 1; lp.btype = g.btype; lp.lb = g.lb; lp.ub = g.ub; }      // (the replay starts from theta, the untouched initial values: it transforms them itself)
        rc = launched("matrix-product nuts (literal replay)", mi::launch_literal(2, lp, rp.n_wg, st));
        if (rc) return rc;
        if (g.n_exec && (rc = copy_flagged_counts(rp.flag, g.n_leap, g.n_exec, C, st))) return rc;      // a replayed chain executed every leapfrog it counts
    }
    mi::note_kernel("%s", kname);
    return finish(chains, d, settings, sc, st, NO_LEAP_FILL, true, n_total);      // (the mass tables are ours)
}

namespace {
// The memoised kernel (nuts_memo.hpp; gt: its DIAGM form with the two mass tables of a diagonal precond_mat), whose name last_kernel() keeps.  Behind it the general
// variant replays the chains it flagged as non-finite -- with gt's tables or, gt null (the plain case), with identity tables filled into id_tab: it reproduces the
// reference's dense products --, and a replayed chain executed every leapfrog it counts
static int nuts_memo_and_replay(mi::NutsParams& prm, StagedChains& sc, int nt, const GeneralTables* gt, uint32_t* nf_flag, double* id_tab, uint32_t nuts_batch, hipStream_t st)
{
    const uint64_t C = prm.C;
    HIP_TRY(hipMemsetAsync(nf_flag, 0, (C + 1) * sizeof(uint32_t), st));
    prm.nf_flag = nf_flag;
    if (gt) { prm.m_sqrt = gt->ms_dev.as<double>(); prm.m_inv = gt->mi_dev.as<double>(); }
    prm.n_exec = sc.dev.n_leapfrogs_executed; sc.exec_written = prm.n_exec != nullptr;
    int rc = launched("nuts", mi::launch_nuts_gauss_memo(prm, nt, st, gt != nullptr));
    if (rc) return rc;
    const std::string reg_name = mi::host::last_kernel();
    mi::NutsParams rp = prm;
    rp.n_exec = nullptr;
    rp.nf_flag = nullptr; rp.replay_flag = nf_flag;
    if (gt) { rp.btype = gt->bt.as<int>(); rp.lb = gt->lb.as<double>(); rp.ub = gt->ub.as<double>(); }
    else {
        int* bt_i = reinterpret_cast<int*>(id_tab);
        hipLaunchKernelGGL(fill_identity_tables_kernel, dim3(1), dim3(128), 0, st, bt_i, id_tab + 128, id_tab + 256, id_tab + 384, id_tab + 512, 128u);
        HIP_TRY(hipGetLastError());
        rp.btype = bt_i; rp.lb = id_tab + 128; rp.ub = id_tab + 256; rp.m_sqrt = id_tab + 384; rp.m_inv = id_tab + 512;
    }
    rp.vals_bound = 0;
    rc = launched("nuts (replay)", mi::launch_nuts_gauss(rp, nt, true, false, false, nuts_batch, st));
    mi::host::last_kernel() = reg_name;
    if (!rc && prm.n_exec) rc = copy_flagged_counts(nf_flag, prm.n_leap, prm.n_exec, C, st);
    return rc;
}

// nuts on the Gaussian kinds with d <= 128, max_tree_depth <= 10: the tile kernels -- the memoised trajectory (nuts_memo.hpp; plain or a diagonal precond_mat alone),
// its bounded form (nuts_bounded_launch.hip), the asynchronous general variants (nuts_async.hpp: a dense precond_mat, the hints)
static int run_nuts_tile(const mi_target* target, const mi_settings* settings, mi_chains* chains, hipStream_t st)
{
    int rc;
    const uint64_t d = target->d;
    const uint64_t n_total = settings->n_burnin_draws + settings->n_keep_draws;
    StagedTarget tg;
    if ((rc = stage_target(target, tg, st))) return rc;
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st, n_total);
    if (rc) return rc;

    mi::NutsParams prm{};
    fill_common(prm, d, settings, chains, sc);
    prm.P = tg.mat;
    prm.sep_target = target->kind != MI_TARGET_GAUSS_DENSE;     // ISO / DIAG: the general variants (and the replay of flagged chains, which is one) take the gradient element-wise
    const int nt = (int)((d + 15) / 16);
    GeneralTables gt;
    rc = general_tables("nuts", settings, d, gt, true, true);
    if (rc) return rc;
    const bool lockstep = target->kernel_hint == MI_KERNEL_NUTS_LOCKSTEP && chains->draw0 == 0 && !chains->nuts_adapt_state;   // the first-generation kernel, same bits (it exports no adaptation state)
    const bool tick_local = target->kernel_hint == MI_KERNEL_NUTS_TICK_LOCAL;  // the asynchronous kernel without register-carried state
    // the plain case and a diagonal precond_mat alone can run on the memoised trajectory (nuts_memo.hpp)
    const bool memo = (!gt.active || (!gt.dense && !settings->vals_bound)) && !lockstep && !tick_local;
    WsLease ws;
    const size_t d_pad = (d <= 16) ? 16 : (d <= 32) ? 32 : (d <= 64) ? 64 : 128;
    size_t ws_own = (size_t)mi::NUTS_NVEC_ASYNC * d_pad * ((chains->n_chains + 15) / 16 + 4) * 16 * sizeof(double);
    // (the memoised kernel's workspace is sized by the chain slots of its persistent grid; the replay of flagged chains re-uses the same
    //  bytes in the asynchronous kernel's layout afterwards)
    if (memo) ws_own = std::max(ws_own, mi::nuts_memo_workspace_bytes(chains->n_chains, nt, gt.active));
    // bounds (with the identity or a diagonal precond_mat): the memoised tick with the tile route's policy (nuts_bounded_launch.hip)
    const bool bounded_memo = gt.active && !gt.dense && settings->vals_bound && !lockstep && !tick_local;
    if (bounded_memo) ws_own = std::max(ws_own, mi::nuts_bounded_workspace_bytes(chains->n_chains, nt));
    const size_t ws_own_r = (ws_own + 255) & ~(size_t)255;
    const size_t flag_bytes = ((chains->n_chains + 1) * sizeof(uint32_t) + 255) & ~(size_t)255;   // [C] flags, [C] "any"
    const size_t fixed_bytes = ws_own_r + flag_bytes + 5 * 128 * sizeof(double) + 256 + 256;     // + non-finite flags + identity tables of the replay + the chain counter
    // The memoised kernel reads the momenta of the whole run from a table its launcher fills first (nuts_memo.hpp: nuts_momenta_kernel) when that table
    // is affordable: at most MI_NUTS_MOMENTA_MAX_BYTES and a third of the device memory that is free right now; else -- and under
    // MI_KERNEL_NUTS_MEMO_INTICK -- the momenta are generated inside the tick, as in rounds 2-5.  Same bits either way.
    size_t mom_bytes = 0;
    if (memo && !gt.active && target->kernel_hint != MI_KERNEL_NUTS_MEMO_INTICK) {          // (the plain case; with a diagonal precond_mat: in the tick, nuts_launch.hip)
        const size_t want = mi::nuts_memo_momenta_bytes(chains->n_chains, (uint32_t)n_total, nt);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        const size_t cached = ws_cached_bytes(st);       // (what this stream's workspace already holds counts as free: it is re-used)
        if (want <= MI_NUTS_MOMENTA_MAX_BYTES && want <= (free_b + cached) / 3) mom_bytes = (want + 255) & ~(size_t)255;
    }
    const size_t split_bytes = (memo || bounded_memo) ? ((mi::nuts_split_workspace_bytes(chains->n_chains, (uint32_t)d) + 255) & ~(size_t)255) : 0;      // (nuts_launch.hip: runs cut into pieces)
    rc = ws_get(st, fixed_bytes + mom_bytes + split_bytes, ws);
    if (rc) return rc;     // every workspace vector is stored by the kernel before it is loaded: no memset needed
    prm.ws = ws.as<double>();
    if (split_bytes) prm.split_ws = static_cast<char*>(ws.p) + fixed_bytes + mom_bytes;
    if (mom_bytes) {
        prm.mom = reinterpret_cast<double*>(static_cast<char*>(ws.p) + fixed_bytes);
        prm.msc = prm.mom + (size_t)n_total * chains->n_chains * (size_t)(16 * (nt <= 1 ? 1 : nt == 2 ? 2 : nt <= 4 ? 4 : 8));
    }
    uint32_t* const nf_flag = reinterpret_cast<uint32_t*>(static_cast<char*>(ws.p) + ws_own_r);
    double* const id_tab = reinterpret_cast<double*>(static_cast<char*>(ws.p) + ws_own_r + flag_bytes);
    prm.next_chain = reinterpret_cast<uint32_t*>(static_cast<char*>(ws.p) + ((ws_own_r + flag_bytes + 5 * 128 * sizeof(double) + 255) & ~(size_t)255));
    prm.n_leap = sc.dev.n_leapfrogs;
#ifdef MI_PROFILING
    DevBuf prof_buf;
    if (getenv("MI_NUTS_PROF")) { HIP_TRY(prof_buf.alloc(96 * 8)); HIP_TRY(hipMemset(prof_buf.p, 0, 96 * 8)); prm.prof = prof_buf.as<unsigned long long>();
}
#endif
    // continuation (checkpoint / resume): the step sizes come back in; inside the adaptation window also the dual-averaging state.
    // (The lock-step hint cannot be honoured for a continuation -- that kernel keeps no per-chain step size: as mi_mcmc.h promises for a
    //  hint the request cannot take, it is ignored and the default kernel runs; it also clamps the window to the call, nuts.cpp:54, which is
    //  the same thing for the single call it serves.)
    if ((rc = fill_nuts(prm, settings, chains, sc))) return rc;
    prm.eps_bar0 = settings->step_size;

    uint32_t nuts_batch = 8;                 // momentum-refresh batch of the asynchronous kernel
#ifdef MI_PROFILING
    if (const char* e = getenv("MI_NUTS_BATCH")) nuts_batch = (uint32_t)atoi(e);
#endif
    if (gt.active && gt.dense) {
        prm.btype = gt.bt.as<int>(); prm.lb = gt.lb.as<double>(); prm.ub = gt.ub.as<double>();
        prm.m_sqrt = gt.ms_dev.as<double>(); prm.m_inv = gt.mi_dev.as<double>();
        prm.Minv = gt.minv_full.as<double>(); prm.Lchol = gt.l_full.as<double>();
        prm.vals_bound = settings->vals_bound ? 1 : 0;
        rc = launched("nuts", mi::launch_nuts_gauss(prm, nt, true, true, false, nuts_batch, st));
        if (!rc) HIP_TRY(hipStreamSynchronize(st));     // the tables are ours
    }
    else if (gt.active && memo) {
        // a diagonal precond_mat alone: the plain-case kernel with two mass tables (nuts_memo.hpp, DIAGM); flagged chains are replayed
        // by the general variant with the same tables
        rc = nuts_memo_and_replay(prm, sc, nt, &gt, nf_flag, id_tab, nuts_batch, st);
        if (!rc) HIP_TRY(hipStreamSynchronize(st));     // the tables are ours
    }
    else if (gt.active) {
        prm.btype = gt.bt.as<int>(); prm.lb = gt.lb.as<double>(); prm.ub = gt.ub.as<double>();
        prm.m_sqrt = gt.ms_dev.as<double>(); prm.m_inv = gt.mi_dev.as<double>();
        prm.vals_bound = settings->vals_bound ? 1 : 0;
        if (bounded_memo) {
            prm.n_exec = sc.dev.n_leapfrogs_executed; sc.exec_written = prm.n_exec != nullptr;
            rc = launched("nuts", mi::launch_nuts_gauss_bounded(prm, nt, st));
        }
        else rc = launched("nuts", mi::launch_nuts_gauss(prm, nt, true, false, false, nuts_batch, st));     // (MI_KERNEL_NUTS_TICK_LOCAL: the tick-local general kernel)
        if (!rc) HIP_TRY(hipStreamSynchronize(st));     // the tables are ours
    }
    else if (lockstep || tick_local) rc = launched("nuts", mi::launch_nuts_gauss(prm, nt, false, false, lockstep, nuts_batch, st));
    else {
        // the plain case: nuts_gauss_memo_kernel; chains that reach the non-finite regime are flagged there and
        // replayed by the general variant, which reproduces the reference's dense products, with identity tables
        rc = nuts_memo_and_replay(prm, sc, nt, nullptr, nf_flag, id_tab, nuts_batch, st);
    }
    if (rc) return rc;
#ifdef MI_PROFILING
    if (prm.prof) {
        unsigned long long h[16];
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(h, prm.prof, sizeof(h), hipMemcpyDeviceToHost));
        // the marks of nuts_memo_core.hpp (MI_MPROF(k) closes phase k); the tick-local kernel (nuts_async.hpp) fills the first eight with its own phases
        const char* names[12] = {"A phase: rows, momenta ahead", "B origin + kick + drift", "mat-vec + kick + energies", "tests (U-turn, memoised)", "C walk",
                                 "init / search", "E record store", "loop head", "point scalars (n', s', alpha)", "D end of doubling", "-", "-"};
        unsigned long long tot = 0;
        for (int k = 0; k < 10; ++k) tot += h[k];            // (slot 10 of the memoised tick is a count: chain-ticks that compute a point)
        for (int k = 0; k < 10; ++k) if (h[k]) fprintf(stderr, "[nuts prof] %-32s %12llu cycles %5.1f%%\n", names[k], h[k], 100.0 * h[k] / (tot ? tot : 1));
        fprintf(stderr, "[nuts prof] ticks %llu (%.0f cycles each), active chain-ticks %llu (%.2f of 16 per tick), of them computing a point %llu (%.2f per tick), walk iterations %llu, test iterations %llu\n", h[12],
                (double)tot / (h[12] ? h[12] : 1), h[13], (double)h[13] / (h[12] ? h[12] : 1), h[10], (double)h[10] / (h[12] ? h[12] : 1), h[14], h[15]);
    }
#endif
    return finish(chains, d, settings, sc, st, NO_LEAP_FILL, tg.owns(), n_total);
}
}  // namespace

int mi_mcmc_nuts_run(const mi_target* target, const mi_settings* settings, mi_chains* chains, void* stream)
{
    int rc = check_common(target, settings, chains);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t d = target->d;
    if (target->kind == MI_TARGET_NORMAL_MODEL) return run_small_normal_model("nuts", 2, target, settings, chains, st);
    if (target->kind == MI_TARGET_LOGISTIC) {
        if (d <= (uint64_t)mi::SMALL_MAX_D && settings->max_tree_depth <= 10) return run_small_logistic("nuts", 2, target, settings, chains, st);
        if (d <= 512 && lds_nuts_case(target, settings)) return run_lds_nuts(target, settings, chains, st, mi::LOGIT_TARGET_LOGISTIC);
        GemmNutsPlan plan;
        if (gemm_nuts_case(target, settings, chains, st, plan)) return run_gemm_nuts(target, settings, chains, st, plan);      // d > 512, plain or bounded: memoised trees, two matrix products per tick
        return run_literal("nuts", 2, target, settings, chains, st);
    }
    if (target->kind != MI_TARGET_GAUSS_ISO && target->kind != MI_TARGET_GAUSS_DIAG && target->kind != MI_TARGET_GAUSS_DENSE)
        return fail(MI_ERR_UNSUPPORTED, "nuts: target kind %d not implemented", target->kind);
    // the tiled kernels: d <= 128, max_tree_depth <= 10 (per-level records and scalars are sized for that); beyond, literal.hpp
    if (target->kind == MI_TARGET_GAUSS_DENSE && d > 128 && d <= 512 && lds_nuts_case(target, settings))
        return run_lds_nuts(target, settings, chains, st, mi::LOGIT_TARGET_DENSE);     // P streamed through LDS (nuts_lds.hpp)
    {
        GemmNutsPlan plan;
        if (gemm_nuts_case(target, settings, chains, st, plan)) return run_gemm_nuts(target, settings, chains, st, plan);      // d > 512, plain or bounded: memoised trees, one matrix product per tick (gemm_nuts.hpp)
    }
    if (d > 128 || settings->max_tree_depth > (uint64_t)mi::NUTS_MAX_DEPTH) return run_literal("nuts", 2, target, settings, chains, st);
    const uint64_t n_total = settings->n_burnin_draws + settings->n_keep_draws;
    if (n_total > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "too many draws");
    return run_nuts_tile(target, settings, chains, st);
}

// mcmc::rmhmc (src/rmhmc.cpp:30-287) for many chains of a small-dimensional target with a built-in metric tensor.
int mi_mcmc_rmhmc_run(const mi_target* target, const mi_settings* settings, mi_chains* chains, void* stream)
{
    int rc = check_common(target, settings, chains);
    if (rc) return rc;
    if (target->kind == MI_TARGET_LOGISTIC) {           // Fisher information + prior precision (small_targets.hpp), d <= 4
        if (target->d > 4)                                // beyond the one-lane engine's d x d x d cubes per lane: one workgroup per chain (literal.hpp)
            return run_literal("rmhmc", 4, target, settings, chains, static_cast<hipStream_t>(stream));
        return run_small_logistic("rmhmc", 4, target, settings, chains, static_cast<hipStream_t>(stream));
    }
    // the Gaussian kinds: their (constant) precision is the metric, its derivative zero -- the oracle's orc_target_tensor; literal.hpp
    if (target->kind == MI_TARGET_GAUSS_ISO || target->kind == MI_TARGET_GAUSS_DIAG || target->kind == MI_TARGET_GAUSS_DENSE)
        return run_literal("rmhmc", 4, target, settings, chains, static_cast<hipStream_t>(stream));
    if (target->kind != MI_TARGET_NORMAL_MODEL)
        return fail(MI_ERR_UNSUPPORTED, "rmhmc: target kind %d has no built-in metric tensor on the device path (user targets: include/mi_mcmc_target.hpp)", target->kind);
    return run_small_normal_model("rmhmc", 4, target, settings, chains, static_cast<hipStream_t>(stream));
}

// mcmc::de (ref: src/de.cpp:28-232) for many populations (de.hpp)
void mi_de_settings_default(mi_de_settings* s)
{
    if (!s) return;
    std::memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(mi_de_settings);          // de_settings_t (mcmc_structs.hpp): jumps false, n_pop 100, par_b 1e-4, gammas 1 / 2
    s->jumps = 0;
    s->n_pop = 100;
    s->par_b = 1e-4;
    s->par_gamma_jump = 2.0;
    s->par_gamma = 1.0;
}

int mi_mcmc_de_run(const mi_target* target, const mi_settings* settings, const mi_de_settings* de, mi_populations* pops, void* stream)
{
    return mi::host::de_run(target, settings, de, pops, static_cast<hipStream_t>(stream));
}

int mi_mcmc_de_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel, void* target_data,
                            const mi_settings* settings, const mi_de_settings* de, double* draws_out, uint64_t* n_accept)
{
    return mi::host::de_run_callback(initial_vals, d, target_log_kernel, target_data, settings, de, draws_out, n_accept);
}

// mcmc::aees (ref: src/aees.cpp:28-305) for many runs (aees.hpp)
void mi_aees_settings_default(mi_aees_settings* s)
{
    if (!s) return;
    std::memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(mi_aees_settings);        // aees_settings_t (mcmc_structs.hpp): n_initial 1000, par_scale 1, n_rings 5, ee_prob 0.1
    s->n_initial_draws = 1000;
    s->par_scale = 1.0;
    s->cov_mat = nullptr;
    s->n_rings = 5;
    s->ee_prob_par = 0.10;
    s->temper_vec = nullptr;
    s->temper_len = 0;
}

int mi_mcmc_aees_run(const mi_target* target, const mi_settings* settings, const mi_aees_settings* aees, mi_aees_runs* runs, void* stream)
{
    return mi::host::aees_run(target, settings, aees, runs, static_cast<hipStream_t>(stream));
}

int mi_mcmc_aees_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel, void* target_data,
                              const mi_settings* settings, const mi_aees_settings* aees, double* draws_out, double* final_states,
                              uint64_t* n_accept, uint64_t* n_ee_accept)
{
    return mi::host::aees_run_callback(initial_vals, d, target_log_kernel, target_data, settings, aees, draws_out, final_states, n_accept, n_ee_accept);
}

}  // extern "C"
