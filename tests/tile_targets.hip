// tests/tile_targets.hip -- the tile-route tests' own target library (tests/tile_route.py builds it the way a user builds
// examples/user_tile_target.hip): the twisted Gaussian of the example, same arithmetic, at the NT / WPB instantiations the example
// does not compile.
//
// TwistedTileN<NT, WPB>  u = v except u_1 = v_1 + b (v_0^2 - s^2),  log K(v) = -1/2 u' P u,  grad = -J' (P u);  2 <= d <= 16 NT.
//     twisted1  NT 1, WPB 4  (d <= 16)       twisted2  NT 2, WPB 4  (d <= 32)       twisted8  NT 8, WPB 8  (d <= 128)
//     (NT 4 is the example's own TwistedTile.)  Three instantiations, six kernels each: the list stays this short on purpose.
// twisted_host_kernel_n  the same target as the reference's host callback for every d <= 128, the operation order of the example's
//     twisted_host_kernel: rows of P u as fma chains with k ascending, the quadratic form as four strided fma chains combined
//     (q0 + q2) + (q1 + q3).  target_data points to a TwistedTileN (any NT: one layout) whose P is a HOST pointer.
#include "mi_mcmc_tile_target.hpp"

template <int NT_, int WPB_>
struct TwistedTileN {
    static constexpr int NT = NT_;
    static constexpr int WPB = WPB_;
    const double* P;        // device (kernels) / host (twisted_host_kernel_n), d x d row-major
    uint32_t d;             // >= 2
    double b, s2;
    size_t lds_doubles() const { return mi::tile::matrix_doubles<NT>(); }
    __device__ void stage(double* lds) const { mi::tile::stage_matrix<NT>(P, d, lds); }
    __device__ void grad_tile(const double* lds, const double (&v)[4 * NT], double (&g)[4 * NT], double& value, bool want_value) const
    {
        const int lane = threadIdx.x & 63;
        // dimension 0 sits in register 0 of the lanes with (lane >> 4) == 0, dimension 1 in register 0 of (lane >> 4) == 1
        const double v0 = __shfl(v[0], lane & 15);
        double u[4 * NT];
#pragma unroll
        for (int s = 0; s < 4 * NT; ++s) u[s] = v[s];
        if ((lane >> 4) == 1) u[0] = v[0] + b * (v0 * v0 - s2);
        double w[4 * NT];
        mi::tile::matvec<NT>(lds, u, w);
        if (want_value) value = -0.5 * mi::tile::dot<4 * NT>(u, w);
        const double w1 = __shfl(w[0], 16 + (lane & 15));
#pragma unroll
        for (int s = 0; s < 4 * NT; ++s) g[s] = -w[s];
        if ((lane >> 4) == 0) g[0] = -(w[0] + ((2.0 * b) * v0) * w1);
    }
};

using Twisted1 = TwistedTileN<1, 4>;
using Twisted2 = TwistedTileN<2, 4>;
using Twisted8 = TwistedTileN<8, 8>;
MI_MCMC_DEFINE_TILE_TARGET(twisted1, Twisted1)
MI_MCMC_DEFINE_TILE_TARGET(twisted2, Twisted2)
MI_MCMC_DEFINE_TILE_TARGET(twisted8, Twisted8)

extern "C" double twisted_host_kernel_n(const double* vals, double* grad_out, void* target_data)
{
    const Twisted8& t = *static_cast<const Twisted8*>(target_data);
    const uint32_t d = t.d;
    double u[128], w[128];
    for (uint32_t i = 0; i < d; ++i) u[i] = vals[i];
    u[1] = vals[1] + t.b * (vals[0] * vals[0] - t.s2);
    for (uint32_t i = 0; i < d; ++i) {
        double acc = 0.0;
        for (uint32_t k = 0; k < d; ++k) acc = __builtin_fma(t.P[(size_t)i * d + k], u[k], acc);
        w[i] = acc;
    }
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = 0; i < d; ++i) q[i & 3] = __builtin_fma(u[i], w[i], q[i & 3]);
    const double value = -0.5 * ((q[0] + q[2]) + (q[1] + q[3]));
    if (grad_out) {
        for (uint32_t i = 0; i < d; ++i) grad_out[i] = -w[i];
        grad_out[0] = -(w[0] + ((2.0 * t.b) * vals[0]) * w[1]);
    }
    return value;
}
