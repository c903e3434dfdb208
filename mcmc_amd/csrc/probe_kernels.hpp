// probe_kernels.hpp -- the math and normals probes of libmi_mcmc_probes.so, written once and compiled by two translation units: probes.hip with
// det_math.hpp as most kernels build it (MI_KC_MODE 1) and probes_kc2.hip as the logistic units build it (MI_KC_MODE 2, MI_RNG_NOINLINE).  The
// template parameter is that mode; it only keeps the two units' kernels apart by name.  Include after det_math.hpp and host_common.hpp.
#pragma once

namespace mi {
namespace probe {

// fn: 0 exp, 1 log, 2 sincos2pi (out = sin, out2 = cos), 3 softplus, 4 sigmoid, 5 norm_ppf
template <int MODE>
__global__ void math_kernel(int fn, const double* x, uint64_t n, double* out, double* out2)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0, c = 0.0;
    switch (fn) {
    case 0: s = mi::det_exp(x[i]); break;
    case 1: s = mi::det_log(x[i]); break;
    case 2: mi::det_sincos2pi(x[i], s, c); break;
    case 3: s = mi::softplus(x[i]); break;
    case 4: s = mi::sigmoid(x[i]); break;
    case 5: s = mi::norm_ppf(x[i]); break;
    default: s = __builtin_nan("");
    }
    out[i] = s;
    out2[i] = c;
}

// fn: 0 det_pow(x, y)
template <int MODE>
__global__ void math2_kernel(int fn, const double* x, const double* y, uint64_t n, double* out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fn == 0 ? mi::det_pow(x[i], y[i]) : __builtin_nan("");
}

// the two normals of one slot into their dimensions (i = 8b + 4h + j <- slot 4b + j, component h); a slot past the last dimension stores nothing
__device__ __forceinline__ void store_slot(uint64_t slot, double z0, double z1, uint64_t d, double* out)
{
    const uint64_t i0 = 8 * (slot / 4) + slot % 4, i1 = i0 + 4;
    if (i0 < d) out[i0] = z0;
    if (i1 < d) out[i1] = z1;
}

// The d normals of one (chain, draw), one thread per group of slots.  variant 0: rng_normal_pair, a thread per slot; 1: rng_normal_pair_at with
// base 4b and j = slot % 4, as the MFMA-layout kernels call it; 2: rng_normal_two_pairs on (slot, slot + 4) and 3: rng_normal_four_pairs on
// slot, slot + 4, slot + 8, slot + 12, as logistic_lds.hpp calls them.
template <int MODE>
__global__ void normals_kernel(int variant, uint64_t seed, uint64_t chain, uint32_t draw, uint32_t stream, uint64_t d, double* out)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nslots = 4 * ((d + 7) / 8);
    if (variant == 0 || variant == 1) {
        if (t >= nslots) return;
        double z0, z1;
        if (variant == 0) mi::rng_normal_pair(seed, chain, draw, (uint32_t)t, stream, z0, z1);
        else mi::rng_normal_pair_at(seed, chain, draw, (uint32_t)(4 * (t / 4)), (uint32_t)(t % 4), stream, z0, z1);
        store_slot(t, z0, z1, d, out);
    } else if (variant == 2) {
        const uint64_t slot = 8 * (t / 4) + t % 4;
        if (slot >= nslots) return;
        const mi::rng_double4 z = mi::rng_normal_two_pairs(seed, chain, draw, (uint32_t)slot, (uint32_t)slot + 4u, stream);
        store_slot(slot, z[0], z[1], d, out);
        store_slot(slot + 4, z[2], z[3], d, out);
    } else {
        const uint64_t slot = 16 * (t / 4) + t % 4;
        if (slot >= nslots) return;
        const mi::rng_double8 z = mi::rng_normal_four_pairs(seed, chain, draw, (uint32_t)slot, 4u, stream);
        for (int k = 0; k < 4; ++k) store_slot(slot + 4 * (uint64_t)k, z[2 * k], z[2 * k + 1], d, out);
    }
}

template <int MODE>
int run_math(int fn, const double* x, uint64_t n, double* out, double* out2)
{
    if (!x || !out || !out2) return mi::host::fail(MI_ERR_BAD_ARG, "null buffer");
    mi::host::DevBuf dx, d1, d2;
    HIP_TRY(dx.alloc(n * 8)); HIP_TRY(d1.alloc(n * 8)); HIP_TRY(d2.alloc(n * 8));
    HIP_TRY(hipMemcpy(dx.p, x, n * 8, hipMemcpyHostToDevice));
    if (n) hipLaunchKernelGGL(math_kernel<MODE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, dx.as<double>(), n, d1.as<double>(), d2.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d1.p, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out2, d2.p, n * 8, hipMemcpyDeviceToHost));
    return MI_OK;
}

template <int MODE>
int run_math2(int fn, const double* x, const double* y, uint64_t n, double* out)
{
    if (!x || !y || !out) return mi::host::fail(MI_ERR_BAD_ARG, "null buffer");
    mi::host::DevBuf dx, dy, d1;
    HIP_TRY(dx.alloc(n * 8)); HIP_TRY(dy.alloc(n * 8)); HIP_TRY(d1.alloc(n * 8));
    HIP_TRY(hipMemcpy(dx.p, x, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dy.p, y, n * 8, hipMemcpyHostToDevice));
    if (n) hipLaunchKernelGGL(math2_kernel<MODE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, dx.as<double>(), dy.as<double>(), n, d1.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d1.p, n * 8, hipMemcpyDeviceToHost));
    return MI_OK;
}

template <int MODE>
int run_normals(int variant, uint64_t seed, uint64_t chain, uint32_t draw, uint32_t stream, uint64_t d, double* out)
{
    if (!out || d == 0 || d > (1ull << 24) || variant < 0 || variant > 3) return mi::host::fail(MI_ERR_BAD_ARG, "bad args");
    mi::host::DevBuf o;
    HIP_TRY(o.alloc(d * 8));
    const uint64_t nslots = 4 * ((d + 7) / 8);
    hipLaunchKernelGGL(normals_kernel<MODE>, dim3((unsigned)((nslots + 63) / 64)), dim3(64), 0, 0, variant, seed, chain, draw, stream, d, o.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, o.p, d * 8, hipMemcpyDeviceToHost));
    return MI_OK;
}

}  // namespace probe
}  // namespace mi
