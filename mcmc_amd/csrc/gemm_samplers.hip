// gemm_samplers.hip -- hmc / mala / rwmh for dense-gradient Gaussian targets BEYOND d = 512: one fp64 matrix product per gradient, for ALL chains at once.
//
// Replaces the draw loops of mcmc::internal::hmc_impl (/root/reference/src/hmc.cpp:155-205 with the leapfrog :164-176), mala_impl
// (src/mala.cpp:149-186 with mala_mean_fn :97-125, mala_prop_adjustment include/mcmc/mala.ipp:30-70, dmvnorm include/stats/dmvnorm.hpp:28-54) and
// rwmh_impl (src/rwmh.cpp:123-151) for log K(theta) = -1/2 theta' P theta, identity precond_mat / cov_mat, no bounds, where n_vals is past what the
// register- and LDS-resident kernels hold (hmc_dense.hpp: d <= 128; logistic_lds.hpp: d <= 512) and literal.hpp served at ~1 % of the matrix peak.
//
// Why a matrix product.  The samplers above are lock-step in the chain index: every chain of a draw does the same number of gradient evaluations,
// so the gradients of all C chains at one leapfrog step are W = P Theta with Theta the d x C matrix of positions -- a DGEMM of 2 d^2 C flop over
// 3 d C doubles of state: d / 12 flop per byte, compute-bound from d ~ 150 on.  Beyond d = 512 the state of a 16-chain tile no longer fits a
// workgroup's registers, and with 288 GB of HBM it does not have to: Theta, the momenta and the gradients live in HBM as [dimension][chain]
// (chains contiguous -- the layout of mi_chains.theta, and the row-major B operand of the product), and one launch per leapfrog step streams them once.
//
//   gemm_step_kernel<MODE>: 128 x 128 output tile per workgroup of four waves (64 x 64 per wave: 16 accumulators of v_mfma_f64_16x16x4_f64), K in steps
//   of 16 through a double-buffered LDS stage that the direct-to-LDS loads (global_load_lds_dwordx4) fill one step ahead -- P is packed TRANSPOSED
//   and zero-padded once per run so that A and B tiles are both rows of 128 contiguous doubles; the LDS row stride of 144 doubles puts the two
//   16-lane groups of a ds_read_b64 on disjoint bank halves.  Element (i, c) of W is ONE fma chain over k ascending (the k-steps of an MFMA and the
//   K loop both ascend): the order of the oracle's orc_gemv and of every other dense kernel of this engine.  The D layout of the instruction (row 4 r + lane / 16)
//   is the B layout, so the epilogue owns whole (dimension, chain) elements and applies, element-wise and with the reference's roundings,
//       MODE 0 = EP_LEAP (a leapfrog step that is not the last): p += (eps g) / 2 (:175), p += (eps g) / 2 (:126 of the NEXT step -- same position, same gradient),
//               theta' = theta + eps p (:171) into the OTHER position buffer (other workgroups still read this one as their B operand);
//       MODE 1 = EP_LAST (the last step): p += (eps g) / 2, W kept for the accept step and as the next draw's first gradient;
//       MODE 2 = EP_GRAD (mala / rwmh / the initial evaluation): W only;
//       MODE 3 = EP_ETA (logistic): eta = X Theta as it is, for gemm_rowterm_kernel to make the row terms of.
//   A DENSE precond_mat (hmc.cpp:57-59,158-160,171,184; mala.cpp:57-58,123,159; mala.ipp:58-64) adds products with INV(M), CHOL_LOWER(M), M and INV(eps^2 M) --
//   the same main loop over matrices packed the same way (upper triangle of CHOL_LOWER: explicit zeros that take part in the chain, as in orc_gemv) -- with
//       MODE 4 = EP_PRODUCT: the product as it is (p = Lc z, mp = Minv p for the kinetic energies, t = M g, Sinv xa, Sinv xb),
//       MODE 5 = EP_DRIFT: the drift theta += eps (Minv p) (:171) -- it leaves the gradient product's epilogue, which becomes
//       MODE 6 = EP_KICKS (a leapfrog step that is not the last): the two half-kicks, no drift,
//       MODE 7 = EP_MALA_PROPOSE (mala): u = Lc z; mean = x + (s2 t) / 2 (mala.cpp:123), proposal = mean + eps u (:159),
//       MODE 8 = EP_MALA_REVERSE (mala): t' = M g'; mean' = x' + (s2 t') / 2, xa = prev - mean', xb = prop - mean (dmvnorm.hpp:37 of both densities):
//   L + 3 products per hmc draw next to the L gradients (2 L + 3 in all), 5 per mala draw next to the one.
//   settings.vals_bound (hmc with the identity / a diagonal precond_mat, rwmh; hmc.cpp:84-95,107-122,134-136,211-218; rwmh.cpp:105-107,113,128): th / thw hold theta, the
//   TRANSFORMED state, and the products are taken at x = inv_transform(theta), a state buffer of its own (xacc / xw[2], double-buffered like thw) that every kernel which
//   moves theta writes next to it.  The Jacobian is diagonal, so the bounded half-kicks are epilogue modes of the gradient's product:
//       MODE 10 = EP_BOX_LEAP (MODE 0 with bounds): p += (eps (J(theta) g)) / 2 twice (:114-122, `jacob_matrix * grad` as the fma chain it is: fma(J_ii, g_i, +0)), theta' = theta + eps (m_inv p),
//               x' = inv_transform(theta') into the OTHER x buffer -- the next product's B operand,
//       MODE 11 = EP_BOX_LAST (MODE 1 with bounds): p += (eps (J(theta) g)) / 2, the RAW gradient (with respect to x) kept: log K(x) and the next draw's first kick are made of it.
//   The tables (bounds type 1..4 of determine_bounds_type.hpp, lb, ub) are read once per 16-row block like m_inv; a block without a bounded dimension (a mask from the host)
//   takes g as it is and x' = theta': no exp, no log.  The energies add log_jacobian(theta) (log_jacobian.hpp:25-58): the terms in parallel, the additions ONE chain over
//   the bounded dimensions ascending.  Kept rows and the final state are the x buffer (:211-218): inv_transform of the accepted theta, the bits the product read.
//   blockIdx -> tile: XCD-aware -- the row tiles of one chain tile run back to back on ONE XCD, so Theta's tile is read from HBM once and shared in that L2.
//
//   Per draw, next to the n_leap products: one kernel per PHASE, the route's VARIANT a template parameter (V_PLAIN: identity / diagonal precond_mat; V_BOX: vals_bound;
//   V_DENSE_M: a dense precond_mat) -- gemm_normals_kernel<V> (Philox + Box-Muller, one slot per thread, canonical slot <-> dimension map of det_math.hpp; mala / rwmh form
//   the proposal there), gemm_pre_kernel<V> (hmc: K = p.(Minv p) / 2 in the engine's four-strided order, first half-kick, first drift) and gemm_post_kernel<ALGO, TGT, V>
//   (energies, accept / reject :186-204, the accepted state and the kept row); gemm_load_kernel<V> and gemm_first_kernel<TGT, V> once per run -- element-wise or one fma
//   chain per (chain, dimension class), HBM-bound, ~5 % of a draw at d = 1024.
//   The launches of one draw are captured ONCE into a hipGraph and replayed n_draws times: the draw index lives in device memory (gemm_advance_kernel).
//
// Reduction orders (the oracle: W = 4, one block; literal.hpp: lit_orders beyond d = 512): dot products as four strided fma chains over dimensions
// j, j + 4, ..., combined (q0 + q2) + (q1 + q3).  Non-finite regime: the element-wise kicks are the reference's dense `inv_precond_matrix * mntm`
// only while everything is finite; a chain whose energies (hmc) / proposal densities (mala) go non-finite is flagged and replayed by literal.hpp.

#include "gemm_samplers.hpp"
#include "launch_common.hpp"      // cap_grid: the test hook's limit on the grid-stride grids
#include "det_math.hpp"
#include "nuts_points.hpp"        // the memoised NUTS trajectory: which points a doubling visits, which tests a point closes (gemm_nuts.hpp)
#include "hmc_dense.hpp"          // box_transform, box_inv_transform, box_inv_jacobian, box_log_jacobian_term: the reference's element-wise maps, out of line

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>

namespace mi {
namespace gemm {

typedef double double4_t __attribute__((ext_vector_type(4)));

#ifndef MI_GEMM_ABLATE
#define MI_GEMM_ABLATE 0          // timing experiments only (results meaningless): 1 no epilogue memory traffic, 2 no tile loads, 4 no barriers
#endif

constexpr int TM = 128, TN = 128, TK = 16;
constexpr int LDS_STRIDE = 144;                      // doubles per staged row: 128 + 16 (k rows j and j + 1 of a fragment read sit 32 banks apart)
constexpr int STAGE = 2 * TK * LDS_STRIDE;           // doubles per stage: 16 rows of the A tile, 16 rows of the B tile
constexpr size_t GEMM_LDS_BYTES = (size_t)2 * STAGE * sizeof(double);

enum : int { TGT_DENSE = 0, TGT_LOGISTIC = 1 };
// the epilogues of gemm_step_kernel (MODE above and in StepParams); the numbers show in the kernels' names (profilers, mi_mcmc_last_kernel()) and stay
enum : int {
    EP_LEAP = 0, EP_LAST = 1, EP_GRAD = 2, EP_ETA = 3,
    EP_PRODUCT = 4, EP_DRIFT = 5, EP_KICKS = 6, EP_MALA_PROPOSE = 7, EP_MALA_REVERSE = 8,
    EP_BOX_LEAP = 10, EP_BOX_LAST = 11,
    EP_NUTS = 12, EP_NUTS_BOX = 13
};

// One product D = A B over K: A^T as [Kp][ldA] (k-major: a row holds the 128 output rows of a tile contiguously), B as [Kp][Cp]
struct StepParams {
    const double* At;        // dense: P^T; logistic: X^T (MODE 3, eta = X Theta) or X itself (X^T r: K runs over the data rows)
    const double* Bm;        // dense: the positions; logistic: the positions (MODE 3) or the row terms y - sigmoid(eta)
    uint32_t Kp, ldA, M_store, n_ntiles;      // K extent (multiple of 16), padded output rows (multiple of 128), output rows that exist in memory
    uint64_t Cp;
    double eps;
    const double* pos;       // MODE 0..2: the positions the gradient is taken at (the logistic gradient subtracts them; MODE 0 drifts them)
    double* pos_out;         // MODE 0
    double* pm;              // MODE 0 / 1
    double* g_out;           // MODE 1 / 2: grad log K
    const double* m_inv;     // MODE 0: diagonal of INV(precond_mat) per dimension (ones: the identity -- 1.0 * p is p, bit for bit)
    double* term_out;        // MODE 3: eta = X Theta [rows padded to 16][Cp] (gemm_rowterm_kernel turns it into the row terms)
    // a dense precond_mat.  MODE 4: g_out = the product.  MODE 5: pos_out = pos + eps * product.  MODE 7: aux0 = t; g_out = mean, pos_out = the proposal.
    // MODE 8: pos = the proposal, aux0 = the accepted state, aux1 = its mean; g_out = xa, pos_out = xb
    const double* aux0;
    const double* aux1;
    double s2;
    // settings.vals_bound.  MODE 10 / 11: pos = theta (the transformed state), Bm = xpos = inv_transform(theta); MODE 10: x_out = inv_transform(pos_out)
    const double* xpos;
    double* x_out;
    const int* bt;           // [dK] bounds type 1..4, lower and upper bound per dimension (type 1, zeros in the padding)
    const double* lb;
    const double* ub;
    const uint32_t* box_blocks;   // [dK / 16] nonzero: the 16-row block holds a bounded dimension
    // nuts (gemm_nuts.hpp).  MODE 12: every chain has its own signed step and takes a point this tick or does not
    const double* ecol;           // [Cp] the step of the column's chain (0: an evaluation without a kick)
    const uint32_t* colmode;      // [Cp] zero: the column's chain takes no point this tick -- its memory stays as it is
    // MODE 13 (MODE 12 with bounds): pos = theta of the point (the transformed state), Bm = xpos = inv_transform(theta), the tables of MODE 10 / 11
};

template <int MODE, int TGT>
__global__ MI_NO_DS_MERGE __launch_bounds__(256, 2) void gemm_step_kernel(const StepParams prm)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane >> 4, c16 = lane & 15;
    // consecutive workgroup ids go round the 8 XCDs: XCD x takes chain tiles x, x + 8, ... and runs their row tiles back to back
    const uint32_t MT = prm.ldA / TM;
    const uint32_t xcd = blockIdx.x & 7u, q = blockIdx.x >> 3;
    const uint32_t nt = xcd + 8u * (q / MT), mt = q % MT;
    if (nt >= prm.n_ntiles) return;
    const size_t m0 = (size_t)mt * TM, n0 = (size_t)nt * TN;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double*)lds;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    // wave w moves rows w, w + 4, ... of the 32 staged rows (0..15: A^T rows k, columns m0..; 16..31: B rows k, chains n0..), 1 KiB each
    auto issue = [&](uint32_t kb, int stage) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = wave + 4 * i;
            const int rr = r & 15;
            const double* src = (i >= 4) ? prm.Bm + ((size_t)(kb * TK + rr) * prm.Cp + n0) : prm.At + ((size_t)(kb * TK + rr) * prm.ldA + m0);
            const uint32_t dst = lds_base + (uint32_t)((stage * STAGE + r * LDS_STRIDE) * 8);
            uint32_t m0_saved;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                         : "=&s"(m0_saved) : "v"(lane16), "s"(dst), "s"(src) : "memory");
        }
    };
    double4_t acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
    const int wm = wave >> 1, wn = wave & 1;             // the wave's 64 x 64 quarter of the tile
    const uint32_t nkb = prm.Kp / TK;
    issue(0, 0);
#pragma unroll 1
    for (uint32_t kb = 0; kb < nkb; ++kb) {
        const int stage = (int)(kb & 1u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's rows of step kb landed ...
        if (!(MI_GEMM_ABLATE & 4)) __syncthreads();           // ... everybody's, and nobody still reads the other stage
        if (kb + 1 < nkb && !(MI_GEMM_ABLATE & 2)) issue(kb + 1, stage ^ 1);
        const double* As = lds + stage * STAGE + j * LDS_STRIDE + wm * 64 + c16;
        const double* Bs = lds + stage * STAGE + (TK + j) * LDS_STRIDE + wn * 64 + c16;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { a[t] = As[4 * kk * LDS_STRIDE + 16 * t]; b[t] = Bs[4 * kk * LDS_STRIDE + 16 * t]; }
#pragma unroll
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[ti][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[ni], acc[ti][ni], 0, 0, 0);
        }
    }
    // epilogue: acc[ti][ni][r] is D at row m0 + 64 wm + 16 ti + 4 r + j, chain n0 + 64 wn + 16 ni + c16.  One batch per 16-row block ti: its 32 loads
    // (momentum and position of 16 elements per lane) are issued together, then the arithmetic, then the stores -- element by element the epilogue was a
    // chain of 64 dependent round trips to memory (66 us per tile with the matrix pipe idle: 0.70 instead of 0.89 of the peak for the whole call)
    const double eps = prm.eps;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const size_t row0 = m0 + (size_t)(64 * wm + 16 * ti);
        if (row0 >= prm.M_store || (MI_GEMM_ABLATE & 1)) continue;          // (M_store is a multiple of 16: the block exists or it does not)
        const size_t base = (row0 + (size_t)j) * prm.Cp + n0 + (size_t)(64 * wn + c16);
        auto at = [&](int r, int ni) -> size_t { return base + (size_t)(4 * r) * prm.Cp + (size_t)(16 * ni); };
        if constexpr (MODE == EP_ETA || MODE == EP_PRODUCT) {      // eta = X Theta as it is: gemm_rowterm_kernel makes the row terms of it, at full occupancy
            double* out = MODE == EP_ETA ? prm.term_out : prm.g_out;      // (EP_PRODUCT: a product with a mass matrix, as it is)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) out[at(r, ni)] = acc[ti][ni][r];
        } else if constexpr (MODE == EP_DRIFT) {      // :171: theta += eps (inv_precond_matrix p), the dense matrix
            double xv[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) xv[r][ni] = prm.pos[at(r, ni)];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) prm.pos_out[at(r, ni)] = xv[r][ni] + eps * acc[ti][ni][r];
        } else if constexpr (MODE == EP_MALA_PROPOSE) {      // mala.cpp:123,159 with u = sqrt_precond_matrix z the product
            double xv[4][4], tv[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) { xv[r][ni] = prm.pos[at(r, ni)]; tv[r][ni] = prm.aux0[at(r, ni)]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const size_t idx = at(r, ni);
                    const double mean = xv[r][ni] + (prm.s2 * tv[r][ni]) / 2.0;
                    prm.g_out[idx] = mean;
                    prm.pos_out[idx] = mean + eps * acc[ti][ni][r];
                }
        } else if constexpr (MODE == EP_MALA_REVERSE) {      // mala.ipp:60-64: the mean at the proposal (t' = precond_matrix g' the product) and dmvnorm.hpp:37 twice
            double xv[4][4], bv[4][4], mv[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) { xv[r][ni] = prm.pos[at(r, ni)]; bv[r][ni] = prm.aux0[at(r, ni)]; mv[r][ni] = prm.aux1[at(r, ni)]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const size_t idx = at(r, ni);
                    const double mean_prop = xv[r][ni] + (prm.s2 * acc[ti][ni][r]) / 2.0;
                    prm.g_out[idx] = bv[r][ni] - mean_prop;
                    prm.pos_out[idx] = xv[r][ni] - mv[r][ni];
                }
        } else if constexpr (MODE == EP_NUTS) {      // nuts: the second half-kick of a point (nuts.cpp:139-154), the step per column
            double ec[4], pv[4][4];
            [[maybe_unused]] double xv[4][4];
            bool on[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const size_t col = n0 + (size_t)(64 * wn + 16 * ni + c16);
                ec[ni] = prm.ecol[col];
                on[ni] = prm.colmode[col] != 0u;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    pv[r][ni] = 0.0;
                    if constexpr (TGT == TGT_LOGISTIC) xv[r][ni] = 0.0;
                    if (on[ni]) {
                        pv[r][ni] = prm.pm[at(r, ni)];
                        if constexpr (TGT == TGT_LOGISTIC) xv[r][ni] = prm.pos[at(r, ni)];
                    }
                }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const size_t idx = at(r, ni);
                    const double v = acc[ti][ni][r];
                    double g;
                    if constexpr (TGT == TGT_DENSE) g = -v;                // grad log K = -(P theta)
                    else g = v - xv[r][ni];                                // X^T (y - sigmoid(eta)) - beta
                    if (on[ni]) {
                        prm.pm[idx] = pv[r][ni] + (ec[ni] * g) / 2.0;     // the second half-step of the chain's leapfrog
                        prm.g_out[idx] = g;
                    }
                }
        } else if constexpr (MODE == EP_NUTS_BOX) {  // nuts with bounds: p += (e_c (J(theta) g)) / 2 (nuts.cpp:108-135), the RAW gradient (with respect to x) kept
            const bool boxed = prm.box_blocks[row0 >> 4] != 0u;            // (the same for the whole wave)
            [[maybe_unused]] double xs[4][4];
            double ec[4], pv[4][4], tv[4][4], lo[4] = {0.0, 0.0, 0.0, 0.0}, hi[4] = {0.0, 0.0, 0.0, 0.0};
            int bt[4] = {1, 1, 1, 1};
            bool on[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const size_t col = n0 + (size_t)(64 * wn + 16 * ni + c16);
                ec[ni] = prm.ecol[col];
                on[ni] = prm.colmode[col] != 0u;
            }
            if (boxed) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { const size_t i = row0 + (size_t)(4 * r + j); bt[r] = prm.bt[i]; lo[r] = prm.lb[i]; hi[r] = prm.ub[i]; }
            }
            // two batches of 8 elements per block, as EP_BOX_LEAP / EP_BOX_LAST
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int r = 2 * h; r < 2 * h + 2; ++r)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        pv[r][ni] = 0.0; tv[r][ni] = 0.0;
                        if constexpr (TGT == TGT_LOGISTIC) xs[r][ni] = 0.0;
                        if (on[ni]) {
                            pv[r][ni] = prm.pm[at(r, ni)];
                            if (boxed) tv[r][ni] = prm.pos[at(r, ni)];
                            if constexpr (TGT == TGT_LOGISTIC) xs[r][ni] = prm.xpos[at(r, ni)];
                        }
                    }
#pragma unroll
                for (int r = 2 * h; r < 2 * h + 2; ++r)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        const size_t idx = at(r, ni);
                        const double v = acc[ti][ni][r];
                        double g;
                        if constexpr (TGT == TGT_DENSE) g = -v;            // grad log K at x: -(P x)
                        else g = v - xs[r][ni];                            // X^T (y - sigmoid(eta)) - x
                        double jg = g;                                     // an unbounded block: J = I
                        if (boxed) jg = dfma(box_inv_jacobian(tv[r][ni], bt[r], lo[r], hi[r]), g, 0.0);     // nuts.cpp:121-131
                        if (on[ni]) {
                            prm.pm[idx] = pv[r][ni] + (ec[ni] * jg) / 2.0;    // the second half-step of the chain's leapfrog
                            prm.g_out[idx] = g;
                        }
                    }
            }
        } else if constexpr (MODE == EP_BOX_LEAP || MODE == EP_BOX_LAST) {      // a leapfrog step in the transformed space (hmc.cpp:107-122,171)
            const bool boxed = prm.box_blocks[row0 >> 4] != 0u;            // (the same for the whole wave)
            [[maybe_unused]] double pv[4][4], tv[4][4], xs[4][4], mi[4], lo[4] = {0.0, 0.0, 0.0, 0.0}, hi[4] = {0.0, 0.0, 0.0, 0.0};
            int bt[4] = {1, 1, 1, 1};
            if constexpr (MODE == EP_BOX_LEAP) {
#pragma unroll
                for (int r = 0; r < 4; ++r) mi[r] = prm.m_inv[row0 + (size_t)(4 * r + j)];
            }
            if (boxed) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { const size_t i = row0 + (size_t)(4 * r + j); bt[r] = prm.bt[i]; lo[r] = prm.lb[i]; hi[r] = prm.ub[i]; }
            }
            // two batches of 8 elements per block (the plain modes take 16): theta rides next to the momentum and the calls below keep more alive
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int r = 2 * h; r < 2 * h + 2; ++r)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        pv[r][ni] = prm.pm[at(r, ni)]; tv[r][ni] = prm.pos[at(r, ni)];
                        if constexpr (TGT == TGT_LOGISTIC) xs[r][ni] = prm.xpos[at(r, ni)];
                    }
#pragma unroll
                for (int r = 2 * h; r < 2 * h + 2; ++r)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        const size_t idx = at(r, ni);
                        const double v = acc[ti][ni][r];
                        double g;
                        if constexpr (TGT == TGT_DENSE) g = -v;            // grad log K at x: -(P x)
                        else g = v - xs[r][ni];                            // X^T (y - sigmoid(eta)) - x
                        double jg = g;                                     // an unbounded block: J = I
                        if (boxed) jg = dfma(box_inv_jacobian(tv[r][ni], bt[r], lo[r], hi[r]), g, 0.0);     // :114-122
                        double p = pv[r][ni];
                        p = p + (eps * jg) / 2.0;                          // second half-step of this leapfrog step
                        if constexpr (MODE == EP_BOX_LAST) { prm.pm[idx] = p; prm.g_out[idx] = g; }
                        else {
                            p = p + (eps * jg) / 2.0;                      // first half-step of the next one: same position, same gradient, same Jacobian
                            prm.pm[idx] = p;
                            const double tn = tv[r][ni] + eps * (mi[r] * p);     // :171
                            prm.pos_out[idx] = tn;
                            prm.x_out[idx] = boxed ? box_inv_transform(tn, bt[r], lo[r], hi[r]) : tn;       // :108 of the next step
                        }
                    }
            }
        } else {
            [[maybe_unused]] double pv[4][4], xv[4][4], mi[4];
            if constexpr (MODE == EP_LEAP) {
#pragma unroll
                for (int r = 0; r < 4; ++r) mi[r] = prm.m_inv[row0 + (size_t)(4 * r + j)];
            }
            if constexpr (MODE != EP_GRAD) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) pv[r][ni] = prm.pm[at(r, ni)];
            }
            if constexpr (MODE == EP_LEAP || TGT == TGT_LOGISTIC) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) xv[r][ni] = prm.pos[at(r, ni)];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const size_t idx = at(r, ni);
                    const double v = acc[ti][ni][r];
                    double g;
                    if constexpr (TGT == TGT_DENSE) g = -v;                // grad log K = -(P theta)
                    else g = v - xv[r][ni];                                // X^T (y - sigmoid(eta)) - beta
                    if constexpr (MODE == EP_GRAD) prm.g_out[idx] = g;
                    else {
                        double p = pv[r][ni];
                        p = p + (eps * g) / 2.0;                           // second half-step of this leapfrog step (hmc.cpp:175)
                        if constexpr (MODE == EP_LAST) { prm.pm[idx] = p; prm.g_out[idx] = g; }
                        else {
                            p = p + (eps * g) / 2.0;                       // first half-step of the next one (:126): same position, same gradient
                            prm.pm[idx] = p;
                            if constexpr (MODE == EP_LEAP) prm.pos_out[idx] = xv[r][ni] + eps * (mi[r] * p);   // :171: theta += eps (inv_precond_matrix p), the matrix diagonal
                        }
                    }
                }
        }
    }
}

// M (rows x cols row-major) -> out[k ld + i] = TRANSPOSE ? M[i][k] : M[k][i] for k < Kp, i < ld, zeros outside the matrix
template <bool TRANSPOSE>
__global__ void gemm_pack_kernel(const double* __restrict__ M, uint32_t rows, uint32_t cols, uint32_t Kp, uint32_t ld, double* __restrict__ out)
{
    const size_t n = (size_t)Kp * ld;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const uint32_t k = (uint32_t)(e / ld), i = (uint32_t)(e % ld);
        if (TRANSPOSE) out[e] = (i < rows && k < cols) ? M[(size_t)i * cols + k] : 0.0;
        else out[e] = (k < rows && i < cols) ? M[(size_t)k * cols + i] : 0.0;
    }
}

// the row terms of the logistic target (the oracle's ORC_TARGET_LOGISTIC; softplus / sigmoid of det_math.hpp), in place over eta [nK][Cp]:
// res = y - sigmoid(eta) (what X^T multiplies), term = y eta - log(1 + e^eta) (what the log-likelihood sums); zeros in the padding rows
__global__ __launch_bounds__(256) void gemm_rowterm_kernel(const double* __restrict__ y, uint32_t n_rows, uint32_t nK, uint64_t Cp, double* __restrict__ res, double* __restrict__ term)
{
    const size_t n = (size_t)nK * Cp;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(e / Cp);
        const bool valid = row < n_rows;
        const double yv = valid ? y[row] : 0.0;
        const double eta = valid ? term[e] : 0.0;
        // softplus / sigmoid (det_math.hpp) share e = exp(-|eta|): each of them evaluates it once, on the same argument -- the same bits (logistic_lds.hpp does the same)
        const double ex = det_exp(eta > 0.0 ? -eta : eta);
        const double l1p = det_log(1.0 + ex);
        const double sp = (eta > 0.0) ? (eta + l1p) : l1p;
        const double sg = (eta >= 0.0) ? (1.0 / (1.0 + ex)) : (ex / (1.0 + ex));
        res[e] = valid ? (yv - sg) : 0.0;
        term[e] = valid ? (yv * eta - sp) : 0.0;
    }
}

enum : int { V_PLAIN = 0, V_BOX = 1, V_DENSE_M = 2 };      // identity / diagonal precond_mat | settings.vals_bound (hmc, rwmh) | a dense precond_mat (hmc, mala)

// settings.vals_bound: what the V_BOX instantiations read next to the rest of DrawParams
struct BoxParams {
    const int* bt;           // [dK] bounds type 1..4 (1 in the padding)
    const double* lb;
    const double* ub;
    const uint32_t* blocks;  // [dK / 16] nonzero: the 16-dimension block holds a bounded dimension
    double* xacc;            // [dK][Cp] inv_transform of th: what the products read, the kept rows and the final state
    double* xw;              // ... of thw
};

struct DrawParams {
    int algo, tgt;
    uint32_t d, dK, nK;      // nK: the data rows padded to 16 (logistic)
    uint64_t C, Cp, chain0;
    double* th;              // [dK][Cp] accepted position
    double* gacc;            // grad log K at the accepted position
    double* thw;             // the proposal (hmc: the leapfrog's end point)
    double* gprop;           // grad log K there
    double* pm;              // hmc: momentum
    const double* term;      // logistic: [nK][Cp] y eta - log(1 + e^eta) of the LAST evaluation
    const double* m;         // [dK] the diagonal of precond_mat, its CHOL_LOWER (sqrt) and INV (reciprocal), and of INV(eps^2 M) (mala); ones / 1 / eps^2 for the
    const double* m_sqrt;    //      identity (1.0 * x is x bit for bit, so the identity runs the same statements)
    const double* m_inv;
    const double* s_inv;
    double* prevE;           // [Cp] hmc: prev_U; mala / rwmh: prev_LP
    double* kprev;           // [Cp] hmc: prev_K of the running draw
    uint64_t* nacc;          // [Cp]
    uint32_t* draw_ctr;      // LOCAL index of the running draw
    const double* theta_in;  // [d][C]
    double* theta_out;
    double* draws;           // [n_keep][d][C]
    uint64_t* n_accept;
    uint32_t* nf_flag;
    uint64_t seed;
    uint32_t n_burnin, draw0;
    double eps, s2, rs, log_det, cons_term;
    // a dense precond_mat (dense_m): the products of the draw, [dK][Cp] each
    int dense_m;
    double* zb;              // the normals (hmc: p = Lc z; mala: u = Lc z)
    const double* mp;        // hmc: Minv p of the last kinetic-energy product
    const double *xa, *sa, *xb, *sb;     // mala: prev - mean(prop), INV(Sigma) of it; prop - mean(prev), INV(Sigma) of it
    BoxParams bx;            // V_BOX
};

// ---- what the per-draw kernels share
// One thread per (chain, class j = index mod 4): the engine's dot products and row sums are four strided chains, combined (q0 + q2) + (q1 + q3); a wave
// holds 16 chains x 4 classes (the MFMA B layout: its loads are the epilogue's 128-byte segments), a workgroup four waves.
struct ClassLane { int lane, j; uint64_t c; };
__device__ __forceinline__ ClassLane class_lane()
{
    const int lane = threadIdx.x & 63;
    return {lane, lane >> 4, ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + (lane & 15)};
}
__device__ __forceinline__ double class_sum(double q)
{
    q = q + __shfl_xor(q, 32);
    q = q + __shfl_xor(q, 16);
    return q;
}
// One Philox slot is two dimensions: i = 8 b + 4 h + j <-> slot 4 b + j, component h (det_math.hpp's canonical order: a contract with every other kernel of the engine)
__device__ __forceinline__ void slot_dims(uint32_t slot, uint32_t& da, uint32_t& db) { da = 8u * (slot >> 2) + (slot & 3u); db = da + 4u; }
// ... and its two normals: zeros for a chain that is not live and for a dimension past d
__device__ __forceinline__ void slot_normal_pair(uint64_t seed, uint64_t chain, uint32_t draw, uint32_t slot, uint32_t stream, bool live, uint32_t d, double& z0, double& z1)
{
    uint32_t da, db;
    slot_dims(slot, da, db);
    z0 = 0.0; z1 = 0.0;
    if (live && da < d) rng_normal_pair(seed, chain, draw, slot, stream, z0, z1);
    if (db >= d) z1 = 0.0;
}

// log K at x, given what the evaluation left in memory.  dense: -1/2 x . (P x) with P x = -g; logistic: sum_r [y_r eta_r - log(1 + e^eta_r)] - 1/2 |x|^2
// (the oracle's ORC_TARGET_LOGISTIC: orc_sum over the rows, orc_dot over the dimensions, both four-strided)
template <int TGT>
__device__ __forceinline__ double log_kernel_value(const DrawParams& prm, const double* x, const double* g, uint64_t c, int j)
{
    double q = 0.0;
#pragma unroll 4
    for (uint32_t i = (uint32_t)j; i < prm.dK; i += 4u) {
        const size_t e = (size_t)i * prm.Cp + c;
        const double xv = x[e];
        if constexpr (TGT == TGT_DENSE) q = dfma(xv, -g[e], q); else q = dfma(xv, xv, q);
    }
    q = class_sum(q);
    if constexpr (TGT == TGT_DENSE) return -0.5 * q;
    else {
        double ll = 0.0;
#pragma unroll 4
        for (uint32_t r = (uint32_t)j; r < prm.nK; r += 4u) ll = ll + prm.term[(size_t)r * prm.Cp + c];
        ll = class_sum(ll);
        return ll - 0.5 * q;
    }
}

// log_jacobian(theta) (log_jacobian.hpp:25-58) of chain c: the terms of four dimensions at a time by the four class lanes of the chain, the additions ONE chain over the
// bounded dimensions ascending (type-1 dimensions add nothing, not even a + 0.0), the same in all four lanes.  Every lane of the wave calls it.
__device__ __forceinline__ double box_log_jacobian(const DrawParams& prm, const double* th, uint64_t c, int lane)
{
    const BoxParams& bx = prm.bx;
    const uint32_t j = (uint32_t)lane >> 4;
    double lj = 0.0;
    for (uint32_t b = 0; b < prm.dK / 16u; ++b) {
        if (bx.blocks[b] == 0u) continue;
#pragma unroll
        for (uint32_t s = 0; s < 4u; ++s) {
            const uint32_t i0 = 16u * b + 4u * s, i = i0 + j;
            const double term = box_log_jacobian_term(th[(size_t)i * prm.Cp + c], bx.bt[i], bx.lb[i], bx.ub[i]);
#pragma unroll
            for (uint32_t g = 0; g < 4u; ++g) {
                const double tg = __shfl(term, (lane & 15) + 16 * (int)g);
                if (bx.bt[i0 + g] != 1) lj = lj + tg;
            }
        }
    }
    return lj;
}
// the value the samplers compare at (theta, x): log K(theta), and with bounds box_log_kernel = log K(x) + log_jacobian(theta) (hmc.cpp:84-95), x = inv_transform(theta)
template <int TGT, int V>
__device__ __forceinline__ double target_value(const DrawParams& prm, const double* th, const double* x, const double* g, const ClassLane& t)
{
    if constexpr (V == V_BOX) {
        const double k = log_kernel_value<TGT>(prm, x, g, t.c, t.j);
        return k + box_log_jacobian(prm, th, t.c, t.lane);
    } else return log_kernel_value<TGT>(prm, th, g, t.c, t.j);
}

// the accept decisions.  newE: what prevE becomes on accept (hmc: prop_U; mala / rwmh: prop_LP); flag: the chain left the finite regime (literal.hpp replays it).
// (Out-parameters, not a returned struct: with the struct the compiler tests the negated decision and lays the commit loop out reject-first, 1.6 % of a bounded rwmh draw)
__device__ __forceinline__ bool hmc_accept(double lp, double prop_K, double prev_U, double prev_K, double z, double& newE, bool& flag)       // hmc.cpp:178-191
{
    double prop_U = -lp;                                       // :178
    const bool u_nf = !is_finite(prop_U);
    if (u_nf) prop_U = INF;                                    // :180-182
    flag = u_nf || !is_finite(prop_K);
    const double x = -(prop_U + prop_K) + (prev_U + prev_K);
    const double comp_val = (x < 0.01) ? x : 0.01;             // :188
    newE = prop_U;
    return z < det_exp(comp_val);                              // :191
}
__device__ __forceinline__ bool mala_accept(const DrawParams& prm, double lp, double qa, double qb, double prev_LP, double z, double& newE, bool& flag)      // mala.cpp:162-173
{
    double pl = lp;
    if (!is_finite(pl)) pl = -INF;                             // mala.cpp:164-166
    const double da = prm.cons_term - 0.5 * (prm.log_det + qa);    // dmvnorm.hpp:41
    const double db = prm.cons_term - 0.5 * (prm.log_det + qb);
    flag = !is_finite(da) || !is_finite(db);
    const double x = pl - prev_LP + (da - db);
    const double comp_val = (x < 0.01) ? x : 0.01;             // mala.cpp:170
    newE = pl;
    return z < det_exp(comp_val);                              // :173
}
__device__ __forceinline__ bool rwmh_accept(double lp, double prev_LP, double z, double& newE)       // rwmh.cpp:130-139
{
    double pl = lp;
    if (!is_finite(pl)) pl = -INF;                             // rwmh.cpp:130-132
    const double x = pl - prev_LP;
    const double comp_val = (x < 0.0) ? x : 0.0;               // :136
    newE = pl;
    return z < det_exp(comp_val);                              // :139
}

// the accepted state and the kept row (hmc.cpp:193-204, mala.cpp:175-184, rwmh.cpp:141-149).  V_BOX: x moves with theta, and it is x that leaves (hmc.cpp:211-218)
template <int V>
__device__ __forceinline__ void commit_and_keep(const DrawParams& prm, bool accept, double* out, uint64_t c, int j)
{
    double* const kept = (V == V_BOX) ? prm.bx.xacc : prm.th;
    const double* const prop = (V == V_BOX) ? prm.bx.xw : prm.thw;
#pragma unroll 4
    for (uint32_t i = (uint32_t)j; i < prm.dK; i += 4u) {
        const size_t e = (size_t)i * prm.Cp + c;
        double v;
        if (accept) {
            v = prop[e]; kept[e] = v;
            if constexpr (V == V_BOX) prm.th[e] = prm.thw[e];
            prm.gacc[e] = prm.gprop[e];
        } else v = kept[e];
        if (out != nullptr && i < prm.d) out[(size_t)i * prm.C] = v;
    }
}

// ---- the per-draw kernels: one per phase
// theta ([d][C]) into the padded state, zeros elsewhere.  V_BOX: the initial values through transform (hmc.cpp:134-136, rwmh.cpp:105-107), and the first x
template <int V>
__global__ void gemm_load_kernel(const DrawParams prm)
{
    const size_t n = (size_t)prm.dK * prm.Cp;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = e / prm.Cp, c = e % prm.Cp;
        if constexpr (V == V_BOX) {
            const BoxParams& bx = prm.bx;
            const bool in = i < prm.d && c < prm.C;
            const double t = in ? box_transform(prm.theta_in[i * prm.C + c], bx.bt[i], bx.lb[i], bx.ub[i]) : 0.0;
            prm.th[e] = t;
            bx.xacc[e] = in ? box_inv_transform(t, bx.bt[i], bx.lb[i], bx.ub[i]) : 0.0;
        } else prm.th[e] = (i < prm.d && c < prm.C) ? prm.theta_in[i * prm.C + c] : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *prm.draw_ctr = 0u;
}

// the normals of a draw (hmc.cpp:156, mala.cpp:150, rwmh.cpp:124): one Philox slot per thread.
// V_PLAIN.  hmc: p = sqrt(m) z (:158).  mala: proposal = mala_mean_fn(prev) + eps z (mala.cpp:123,159).  rwmh: proposal = prev + par_scale z (rwmh.cpp:126).
// V_BOX (rwmh; bounded hmc draws its momenta with V_PLAIN): the proposal in the transformed space and x = inv_transform of it, where the target is evaluated
//        (rwmh.cpp:128 with hmc.cpp:84-95).
// V_DENSE_M: the normals as they are -- sqrt_precond_matrix z (hmc.cpp:158, mala.cpp:159) is a product.
template <int V>
__global__ __launch_bounds__(256) void gemm_normals_kernel(const DrawParams prm)
{
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= prm.Cp) return;
    const uint32_t slot = blockIdx.y;
    uint32_t da, db;
    slot_dims(slot, da, db);
    const uint32_t draw = *prm.draw_ctr;
    double z0, z1;
    slot_normal_pair(prm.seed, prm.chain0 + c, draw + prm.draw0, slot, STREAM_NORMAL, c < prm.C, prm.d, z0, z1);
    const size_t ia = (size_t)da * prm.Cp + c, ib = (size_t)db * prm.Cp + c;
    if constexpr (V == V_DENSE_M) {
        prm.zb[ia] = z0;
        prm.zb[ib] = z1;
    } else if constexpr (V == V_BOX) {
        const BoxParams& bx = prm.bx;
        const double ta = prm.th[ia] + prm.eps * z0, tb = prm.th[ib] + prm.eps * z1;
        prm.thw[ia] = ta; prm.thw[ib] = tb;
        const bool boxed = bx.blocks[da >> 4] != 0u;          // (da and db = da + 4 share a 16-dimension block)
        bx.xw[ia] = boxed ? box_inv_transform(ta, bx.bt[da], bx.lb[da], bx.ub[da]) : ta;
        bx.xw[ib] = boxed ? box_inv_transform(tb, bx.bt[db], bx.lb[db], bx.ub[db]) : tb;
    } else if (prm.algo == GEMM_HMC) { prm.pm[ia] = prm.m_sqrt[da] * z0; prm.pm[ib] = prm.m_sqrt[db] * z1; }      // p = sqrt_precond_matrix z (:158), the matrix diagonal
    else if (prm.algo == GEMM_MALA) {                    // mean = x + eps^2 (M grad) / 2 (mala.cpp:123), proposal = mean + eps (sqrt(M) z) (:159)
        prm.thw[ia] = (prm.th[ia] + (prm.s2 * (prm.m[da] * prm.gacc[ia])) / 2.0) + prm.eps * (prm.m_sqrt[da] * z0);
        prm.thw[ib] = (prm.th[ib] + (prm.s2 * (prm.m[db] * prm.gacc[ib])) / 2.0) + prm.eps * (prm.m_sqrt[db] * z1);
    } else {
        prm.thw[ia] = prm.th[ia] + prm.eps * z0;
        prm.thw[ib] = prm.th[ib] + prm.eps * z1;
    }
}

// hmc: prev_K = p . (Minv p) / 2 (hmc.cpp:160), the first half-step (:126) and the first drift (:171) of the draw; new_draw = prev_draw (:162).
// V_BOX: the half-step takes J(theta) g (:114-122), the drift writes x = inv_transform(theta') next to theta'.
// V_DENSE_M: Minv p is the product mp before this kernel, the drift the next product's epilogue.
template <int V>
__global__ __launch_bounds__(256) void gemm_pre_kernel(const DrawParams prm)
{
    const ClassLane t = class_lane();
    const uint64_t c = t.c;
    double q = 0.0;
    constexpr int UNROLL = V == V_BOX ? 1 : 4;           // (the bounded loop calls out of line and was never unrolled)
#pragma unroll UNROLL
    for (uint32_t i = (uint32_t)t.j; i < prm.dK; i += 4u) {
        const size_t e = (size_t)i * prm.Cp + c;
        double p = prm.pm[e];
        if constexpr (V == V_DENSE_M) {
            q = dfma(p, prm.mp[e], q);                           // :160
            p = p + (prm.eps * prm.gacc[e]) / 2.0;               // :126
            prm.pm[e] = p;
        } else if constexpr (V == V_BOX) {
            const BoxParams& bx = prm.bx;
            const bool boxed = bx.blocks[i >> 4] != 0u;
            const double mi = prm.m_inv[i], th = prm.th[e], g = prm.gacc[e];
            q = dfma(p, mi * p, q);                              // K = p . (Minv p) / 2 (:160)
            const double jg = boxed ? dfma(box_inv_jacobian(th, bx.bt[i], bx.lb[i], bx.ub[i]), g, 0.0) : g;
            p = p + (prm.eps * jg) / 2.0;
            prm.pm[e] = p;
            const double tn = th + prm.eps * (mi * p);           // :171
            prm.thw[e] = tn;
            bx.xw[e] = boxed ? box_inv_transform(tn, bx.bt[i], bx.lb[i], bx.ub[i]) : tn;
        } else {
            const double mi = prm.m_inv[i];
            q = dfma(p, mi * p, q);                              // K = p . (Minv p) / 2 (:160)
            p = p + (prm.eps * prm.gacc[e]) / 2.0;
            prm.pm[e] = p;
            prm.thw[e] = prm.th[e] + prm.eps * (mi * p);         // :171
        }
    }
    q = class_sum(q);
    if (t.j == 0) prm.kprev[c] = q / 2.0;
}

// the value at the initial state (hmc.cpp:140, mala.cpp:138, rwmh.cpp:113)
template <int TGT, int V>
__global__ __launch_bounds__(256) void gemm_first_kernel(const DrawParams prm)
{
    const ClassLane t = class_lane();
    const double first_lp = target_value<TGT, V>(prm, prm.th, prm.bx.xacc, prm.gacc, t);
    if (t.j == 0) { prm.prevE[t.c] = (prm.algo == GEMM_HMC) ? -first_lp : first_lp; prm.nacc[t.c] = 0ull; }
}

// the accept step (hmc.cpp:178-204; mala.cpp:162-184 with mala.ipp:59-64 and dmvnorm.hpp:37-41; rwmh.cpp:128-149), the accepted state and the kept row
template <int ALGO, int TGT, int V = V_PLAIN>
__global__ __launch_bounds__(256) void gemm_post_kernel(const DrawParams prm)
{
    static_assert(V != V_BOX || ALGO == GEMM_HMC || ALGO == GEMM_RWMH, "bounds: hmc and rwmh");
    static_assert(V != V_DENSE_M || ALGO == GEMM_HMC || ALGO == GEMM_MALA, "a dense precond_mat: hmc and mala");
    const ClassLane t = class_lane();
    const int j = t.j;
    const uint64_t c = t.c;
    const bool live = c < prm.C;
    const uint32_t draw = *prm.draw_ctr;
    const double lp = target_value<TGT, V>(prm, prm.thw, prm.bx.xw, prm.gprop, t);
    double qk = 0.0, qa = 0.0, qb = 0.0;
    if constexpr (ALGO != GEMM_RWMH) {
#pragma unroll 4
        for (uint32_t i = (uint32_t)j; i < prm.dK; i += 4u) {
            const size_t e = (size_t)i * prm.Cp + c;
            if constexpr (ALGO == GEMM_HMC && V == V_DENSE_M) qk = dfma(prm.pm[e], prm.mp[e], qk);      // :184, mp = Minv p the product before this kernel
            else if constexpr (ALGO == GEMM_HMC) { const double p = prm.pm[e]; qk = dfma(p, prm.m_inv[i] * p, qk); }      // :184
            else if constexpr (V == V_DENSE_M) {                       // dmvnorm.hpp:39 with INV(Sigma) (x - mu) the two products before this kernel
                const double xa = prm.xa[e], xb = prm.xb[e];
                qa = dfma(xa, prm.sa[e], qa);
                qb = dfma(xb, prm.sb[e], qb);
            } else {                                                     // Sigma = eps^2 M: INV(Sigma)_ii from the host (s_inv), the means with M grad
                const double x = prm.thw[e], be = prm.th[e], gr = prm.gacc[e], gp = prm.gprop[e];
                const double mm = prm.m[i], si = prm.s_inv[i];
                const double mean_prop = x + (prm.s2 * (mm * gp)) / 2.0;
                const double xa = be - mean_prop;                      // dmvnorm.hpp:37
                qa = dfma(xa, si * xa, qa);
                const double mean_prev = be + (prm.s2 * (mm * gr)) / 2.0;
                const double xb = x - mean_prev;
                qb = dfma(xb, si * xb, qb);
            }
        }
    }
    const double prevE = prm.prevE[c];
    const double z = rng_uniform(prm.seed, prm.chain0 + (live ? c : 0), draw + prm.draw0, 0u);
    bool accept, flag = false;
    double newE;
    if constexpr (ALGO == GEMM_HMC) {
        qk = class_sum(qk);
        accept = hmc_accept(lp, qk / 2.0, prevE, prm.kprev[c], z, newE, flag);       // prop_K = qk / 2 (:184)
    } else if constexpr (ALGO == GEMM_MALA) {
        qa = class_sum(qa); qb = class_sum(qb);
        accept = mala_accept(prm, lp, qa, qb, prevE, z, newE, flag);
    } else accept = rwmh_accept(lp, prevE, z, newE);
    const bool kept = draw >= prm.n_burnin;
    if (j == 0) {
        if (accept) prm.prevE[c] = newE;
        if (accept && kept) prm.nacc[c] += 1ull;
        if (flag && live && prm.nf_flag) { prm.nf_flag[c] = 1u; prm.nf_flag[prm.C] = 1u; }
    }
    double* out = (kept && prm.draws != nullptr && live) ? prm.draws + (size_t)(draw - prm.n_burnin) * prm.d * prm.C + c : nullptr;
    commit_and_keep<V>(prm, accept, out, c, j);
}

__global__ void gemm_advance_kernel(uint32_t* draw_ctr) { *draw_ctr += 1u; }

// final state and accept counts of the chains that were not flagged (a flagged chain is replayed from theta, which must stay its initial state)
__global__ void gemm_store_kernel(const DrawParams prm)
{
    const size_t n = (size_t)prm.d * prm.C;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = e / prm.C, c = e % prm.C;
        const bool flagged = prm.nf_flag != nullptr && prm.nf_flag[c] != 0u;
        if (!flagged) {
            prm.theta_out[e] = prm.th[i * prm.Cp + c];
            if (i == 0 && prm.n_accept) prm.n_accept[c] = prm.nacc[c];
        }
    }
}

static inline uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }
static inline uint64_t padded_chains(uint64_t C) { return (C + TN - 1) / TN * TN; }

// the padded extents of a run with Cp columns (chains)
struct Layout {
    uint32_t dK, dM, nK, nM;
    uint64_t Cp;
    size_t vec, rvec;      // doubles per state array / per row-term array
};
static Layout layout_of(uint32_t d, uint32_t n_rows, uint64_t Cp)
{
    Layout l;
    l.dK = round_up(d, TK); l.dM = round_up(d, TM);
    l.nK = n_rows ? round_up(n_rows, TK) : 0; l.nM = n_rows ? round_up(n_rows, TM) : 0;
    l.Cp = Cp;
    l.vec = (size_t)l.dK * l.Cp;
    l.rvec = (size_t)l.nK * l.Cp;
    return l;
}
uint32_t gemm_padded_d(uint32_t d) { return round_up(d, TK); }

// ---- the workspace.  Each runner describes its regions ONCE (gemm_carve; gemm_nuts_carve in gemm_nuts.hpp): without a base the description counts (gemm_ws_bytes,
// gemm_nuts_chain_bytes / gemm_nuts_fixed_bytes: what the caller allocates and routes on), with a base it hands out a run's pointers: what is counted is what is bound.
struct Carve {
    double* base;
    size_t n = 0;          // doubles handed out so far
    double* take(size_t doubles) { double* p = base ? base + n : nullptr; n += doubles; return p; }
};
// what the evaluation of the target reads and writes, in both runners
struct TargetWs {
    Layout l;
    double *A1, *A2;       // dense: P^T [dK][dM]; logistic: X^T [dK][nM] and X [nK][dM]
    double *res, *term;    // logistic: the row terms [nK][Cp] (y - sigmoid(eta): what X^T multiplies; y eta - log(1 + e^eta): what the log-likelihood sums)
};
static void take_matrices(Carve& cv, TargetWs& w)
{
    const Layout& l = w.l;
    w.A1 = cv.take((size_t)l.dK * (l.nK ? l.nM : l.dM));
    w.A2 = l.nK ? cv.take((size_t)l.nK * l.dM) : nullptr;
}
static void take_row_terms(Carve& cv, TargetWs& w) { w.res = cv.take(w.l.rvec); w.term = cv.take(w.l.rvec); }

constexpr int DENSE_M_MATS = 3, DENSE_M_VECS = 4;     // hmc: CHOL_LOWER(M), INV(M); mala: M, CHOL_LOWER(M), INV(eps^2 M) | hmc: z, Minv p; mala: z / Sinv xa, t / Sinv xb, mean, xa (xb where hmc keeps p)
struct GemmWs : TargetWs {
    double *th, *gacc, *thw[2], *gprop, *pm;              // [dK][Cp] each (DrawParams)
    double *prevE, *kprev;                                // [Cp]
    uint64_t* nacc;
    uint32_t* draw_ctr;
    double* Mm[DENSE_M_MATS];                             // a dense precond_mat: its matrices packed like P^T [dK][dM] (hmc Lc, Minv; mala M, Lc, Sinv) ...
    double* ev[DENSE_M_VECS];                             // ... and the vectors of its products
    double *xacc, *xw[2];                                 // vals_bound: inv_transform of th / thw[0] / thw[1]
    size_t n_doubles;
};
// matrices | th, gacc, thw0, thw1, gprop, pm | res, term | prevE, kprev, nacc | draw counter | a dense precond_mat's matrices and vectors, or (never both) vals_bound's x
static GemmWs gemm_carve(uint32_t d, uint32_t n_rows, uint64_t C, bool dense_mass, bool bounded, double* base)
{
    GemmWs w{};
    w.l = layout_of(d, n_rows, padded_chains(C));
    const Layout& l = w.l;
    Carve cv{base};
    take_matrices(cv, w);
    w.th = cv.take(l.vec); w.gacc = cv.take(l.vec); w.thw[0] = cv.take(l.vec); w.thw[1] = cv.take(l.vec); w.gprop = cv.take(l.vec); w.pm = cv.take(l.vec);
    take_row_terms(cv, w);
    w.prevE = cv.take(l.Cp); w.kprev = cv.take(l.Cp);
    w.nacc = reinterpret_cast<uint64_t*>(cv.take(l.Cp));
    w.draw_ctr = reinterpret_cast<uint32_t*>(cv.take(32));
    if (dense_mass) {
        for (double*& m : w.Mm) m = cv.take((size_t)l.dK * l.dM);
        for (double*& v : w.ev) v = cv.take(l.vec);
    }
    if (bounded) { w.xacc = cv.take(l.vec); w.xw[0] = cv.take(l.vec); w.xw[1] = cv.take(l.vec); }
    w.n_doubles = cv.n;
    return w;
}
size_t gemm_ws_bytes(uint32_t d, uint32_t n_rows, uint64_t C, bool dense_mass, bool bounded) { return gemm_carve(d, n_rows, C, dense_mass, bounded, nullptr).n_doubles * sizeof(double); }

#define GEMM_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)

// ---- what both runners (gemm_run_t here, gemm_nuts_run_t in gemm_nuts.hpp) do on the host
template <int MODE, int TGT>
static int launch_step(const StepParams& sp, hipStream_t st)
{
    const uint32_t MT = sp.ldA / TM;
    const uint32_t grid = 8u * MT * ((sp.n_ntiles + 7u) / 8u);
    hipLaunchKernelGGL((gemm_step_kernel<MODE, TGT>), dim3(grid), dim3(256), GEMM_LDS_BYTES, st, sp);
    return (int)hipGetLastError();
}
// The instantiations of gemm_step_kernel, listed ONCE, for a run on target TGT: X(mode, target).  (The products with a mass matrix have no target: they exist once;
// eta exists for the logistic target alone)
#define GEMM_STEP_MODES(X, TGT) \
    X(EP_LEAP, TGT) X(EP_LAST, TGT) X(EP_GRAD, TGT) X(EP_KICKS, TGT) X(EP_BOX_LEAP, TGT) X(EP_BOX_LAST, TGT) X(EP_NUTS, TGT) X(EP_NUTS_BOX, TGT) X(EP_ETA, TGT_LOGISTIC) \
    X(EP_PRODUCT, TGT_DENSE) X(EP_DRIFT, TGT_DENSE) X(EP_MALA_PROPOSE, TGT_DENSE) X(EP_MALA_REVERSE, TGT_DENSE)
template <int TGT>
static int step_attrs()      // once per process and target: 73 728 bytes of dynamic LDS are above the 64 KiB default
{
#define GEMM_STEP_ATTR(M, T) if (!e) e = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_step_kernel<M, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_LDS_BYTES);
    static const int rc = [] { int e = 0; GEMM_STEP_MODES(GEMM_STEP_ATTR, TGT) return e; }();
#undef GEMM_STEP_ATTR
    return rc;
}
template <int TGT>
static int launch_step_mode(int mode, const StepParams& sp, hipStream_t st)
{
    switch (mode) {
#define GEMM_STEP_CASE(M, T) case M: return launch_step<M, T>(sp, st);
        GEMM_STEP_MODES(GEMM_STEP_CASE, TGT)
#undef GEMM_STEP_CASE
    }
    return (int)hipErrorInvalidValue;
}

// the grid of a GRID-STRIDE kernel over n elements, 256 per workgroup: at most max_wg workgroups, and at most the test hook's cap (launch_common.hpp) -- the kernel
// loops, so the bits do not depend on it.  Only such kernels take it: the step kernel, the class-wise, normals and prepare kernels index by workgroup id
static unsigned stride_grid(size_t n, size_t max_wg = 65535) { return (unsigned)cap_grid(std::min<size_t>((n + 255) / 256, max_wg)); }
static dim3 pack_grid(size_t n) { return dim3(stride_grid(n)); }
// the target's matrices into the workspace, zero-padded: P^T, or X^T and X
template <int TGT>
static void pack_target(const TargetWs& w, const double* P, const double* X, uint32_t n_rows, uint32_t d, hipStream_t st)
{
    const Layout& l = w.l;
    if constexpr (TGT == TGT_LOGISTIC) {
        hipLaunchKernelGGL(gemm_pack_kernel<true>, pack_grid((size_t)l.dK * l.nM), dim3(256), 0, st, X, n_rows, d, l.dK, l.nM, w.A1);
        hipLaunchKernelGGL(gemm_pack_kernel<false>, pack_grid((size_t)l.nK * l.dM), dim3(256), 0, st, X, n_rows, d, l.nK, l.dM, w.A2);
    } else {
        hipLaunchKernelGGL(gemm_pack_kernel<true>, pack_grid((size_t)l.dK * l.dM), dim3(256), 0, st, P, d, d, l.dK, l.dM, w.A1);
    }
}
// grad log K of every chain at the positions B through the epilogue `mode` (its other operands: `sp`).  dense: one product; logistic: eta = X B, the row terms, then
// X^T (y - sigmoid(eta)) with the rows ascending
template <int TGT>
static int gradient_product(const TargetWs& w, const double* y, uint32_t n_rows, const double* B, int mode, StepParams sp, hipStream_t s)
{
    const Layout& l = w.l;
    if constexpr (TGT == TGT_LOGISTIC) {
        StepParams se = sp;
        se.At = w.A1; se.Bm = B; se.Kp = l.dK; se.ldA = l.nM; se.M_store = l.nK; se.term_out = w.term;
        if (int e = launch_step<EP_ETA, TGT>(se, s)) return e;
        hipLaunchKernelGGL(gemm_rowterm_kernel, dim3(stride_grid(l.rvec, (size_t)1 << 20)), dim3(256), 0, s, y, n_rows, l.nK, l.Cp, w.res, w.term);
        sp.At = w.A2; sp.Bm = w.res; sp.Kp = l.nK; sp.ldA = l.dM; sp.M_store = l.dK;
    } else {
        sp.At = w.A1; sp.Bm = B; sp.Kp = l.dK; sp.ldA = l.dM; sp.M_store = l.dK;
    }
    return launch_step_mode<TGT>(mode, sp, s);
}

// The launches of one draw / one tick captured into a graph and instantiated (false: no graph, the caller enqueues them itself).  Captured on a stream of our own (the
// caller's may be the legacy default stream, which cannot be captured): ONE for the process, so two host threads take turns at it
static bool capture_and_instantiate(const std::function<int(hipStream_t)>& enqueue, hipGraph_t* graph, hipGraphExec_t* exec)
{
    static hipStream_t cap_st = [] { hipStream_t s = nullptr; if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr; return s; }();
    static std::mutex cap_mu;
    std::lock_guard<std::mutex> cap_lk(cap_mu);
    *graph = nullptr; *exec = nullptr;
    if (cap_st != nullptr && hipStreamBeginCapture(cap_st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        const int e = enqueue(cap_st);
        const hipError_t ec = hipStreamEndCapture(cap_st, graph);
        if (e == 0 && ec == hipSuccess && *graph != nullptr && hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0) == hipSuccess) return true;
        if (*exec) (void)hipGraphExecDestroy(*exec);
        if (*graph) (void)hipGraphDestroy(*graph);
        *exec = nullptr; *graph = nullptr;
    }
    (void)hipGetLastError();
    return false;
}
// ... and its end: the executable graph must outlive its launches, however the replay ended, so the stream is drained first.  Returns that wait's status
static int release_graph(hipStream_t st, hipGraph_t graph, hipGraphExec_t exec)
{
    const int rc = (int)hipStreamSynchronize(st);
    (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
    return rc;
}

template <int TGT>
static int gemm_run_t(const GemmRun& r, hipStream_t st, const char** kernel_name)
{
    const bool dm = r.dense_mass, box = r.bounded;
    if (box && (dm || r.algo == GEMM_MALA || !r.btype || !r.lb || !r.ub || !r.box_blocks)) return (int)hipErrorInvalidValue;     // (the caller routes these elsewhere)
    const uint32_t n_rows = TGT == TGT_LOGISTIC ? r.n_rows : 0u;
    const GemmWs w = gemm_carve(r.d, n_rows, r.C, dm, box, static_cast<double*>(r.ws));
    const Layout& l = w.l;
    double* const th = w.th; double* const gacc = w.gacc; double* const gprop = w.gprop; double* const pm = w.pm;
    double* const* thw = w.thw; double* const* xw = w.xw; double* const* ev = w.ev;
    const bool hmc = r.algo == GEMM_HMC;
    const double *A_lc = hmc ? w.Mm[0] : w.Mm[1], *A_minv = w.Mm[1], *A_m = w.Mm[0], *A_sinv = w.Mm[2];

    DrawParams dp{};
    dp.algo = r.algo; dp.tgt = TGT; dp.d = r.d; dp.dK = l.dK; dp.nK = l.nK; dp.C = r.C; dp.Cp = l.Cp; dp.chain0 = r.chain0;
    dp.th = th; dp.gacc = gacc; dp.thw = thw[0]; dp.gprop = gprop; dp.pm = pm; dp.term = w.term; dp.prevE = w.prevE; dp.kprev = w.kprev; dp.nacc = w.nacc; dp.draw_ctr = w.draw_ctr;
    dp.theta_in = r.theta; dp.theta_out = r.theta; dp.draws = r.draws; dp.n_accept = r.n_accept; dp.nf_flag = r.nf_flag;
    dp.seed = r.seed; dp.n_burnin = r.n_burnin; dp.draw0 = r.draw0;
    dp.eps = r.eps; dp.s2 = r.s2; dp.rs = r.rs; dp.log_det = r.log_det; dp.cons_term = r.cons_term;
    dp.dense_m = dm ? 1 : 0; dp.zb = ev[0];
    if (hmc) dp.mp = ev[1]; else { dp.xa = ev[3]; dp.sa = ev[0]; dp.xb = pm; dp.sb = ev[1]; }
    dp.bx.bt = r.btype; dp.bx.lb = r.lb; dp.bx.ub = r.ub; dp.bx.blocks = r.box_blocks; dp.bx.xacc = w.xacc; dp.bx.xw = xw[0];
    dp.m = r.mass_tables; dp.m_sqrt = r.mass_tables + l.dK; dp.m_inv = r.mass_tables + 2 * (size_t)l.dK; dp.s_inv = r.mass_tables + 3 * (size_t)l.dK;

    if (int e = step_attrs<TGT>()) return e;
    const uint32_t n_ntiles = (uint32_t)(l.Cp / TN);
    // grad log K (and, logistic, the row terms) at `pos` through the epilogue `mode` (pos_out: EP_LEAP's next position).  vals_bound, EP_BOX_LEAP / EP_BOX_LAST: `pos` is
    // x = inv_transform(theta), what the products read; theta, theta' and x' ride in th_pos / pos_out / x_out
    auto evaluate = [&](const double* pos, int mode, double* pos_out, double* g_out, hipStream_t s, const double* th_pos = nullptr, double* x_out = nullptr) -> int {
        StepParams sp{};
        sp.n_ntiles = n_ntiles; sp.Cp = l.Cp; sp.eps = r.eps; sp.pm = pm; sp.pos = pos; sp.pos_out = pos_out; sp.g_out = g_out; sp.m_inv = dp.m_inv;
        if (mode == EP_BOX_LEAP || mode == EP_BOX_LAST) { sp.pos = th_pos; sp.xpos = pos; sp.x_out = x_out; sp.bt = r.btype; sp.lb = r.lb; sp.ub = r.ub; sp.box_blocks = r.box_blocks; }
        return gradient_product<TGT>(w, r.y, r.n_rows, pos, mode, sp, s);
    };
    // a product with one of the packed mass matrices ([dK][dM], like P^T), B = `vec`; the epilogue of `mode` (EP_PRODUCT, EP_DRIFT, EP_MALA_PROPOSE, EP_MALA_REVERSE: StepParams)
    auto mass_product = [&](const double* At, const double* vec, int mode, const double* pos, double* pos_out, double* out, const double* aux0, const double* aux1, hipStream_t s) -> int {
        StepParams sp{};
        sp.n_ntiles = n_ntiles; sp.Cp = l.Cp; sp.eps = r.eps; sp.s2 = r.s2; sp.pos = pos; sp.pos_out = pos_out; sp.g_out = out; sp.aux0 = aux0; sp.aux1 = aux1;
        sp.At = At; sp.Bm = vec; sp.Kp = l.dK; sp.ldA = l.dM; sp.M_store = l.dK;
        return launch_step_mode<TGT>(mode, sp, s);
    };

    const unsigned ew_grid = stride_grid(l.vec);
    const unsigned cls_grid = (unsigned)(l.Cp / 64);                 // 4 waves x 16 chains per workgroup
    auto per_chain = [&](void (*kernel)(DrawParams), const DrawParams& p, hipStream_t s) { hipLaunchKernelGGL(kernel, dim3(cls_grid), dim3(256), 0, s, p); };
    pack_target<TGT>(w, r.P, r.X, r.n_rows, r.d, st);
    if (dm) {                                                          // (the mass matrices arrive TRANSPOSED, as the literal replay reads them: row k of the pack is row k of them)
        const double* src[DENSE_M_MATS] = {hmc ? r.Lc_t : r.M_t, hmc ? r.Minv_t : r.Lc_t, hmc ? nullptr : r.Sinv_t};
        for (int i = 0; i < DENSE_M_MATS; ++i)
            if (src[i]) hipLaunchKernelGGL(gemm_pack_kernel<false>, pack_grid((size_t)l.dK * l.dM), dim3(256), 0, st, src[i], r.d, r.d, l.dK, l.dM, w.Mm[i]);
    }
    // the initial values (vals_bound: x = inv_transform(transform(them)), hmc.cpp:134-140), the evaluation there
    hipLaunchKernelGGL(box ? gemm_load_kernel<V_BOX> : gemm_load_kernel<V_PLAIN>, dim3(ew_grid), dim3(256), 0, st, dp);
    if (int e = evaluate(box ? w.xacc : th, EP_GRAD, nullptr, gacc, st)) return e;
    per_chain(box ? gemm_first_kernel<TGT, V_BOX> : gemm_first_kernel<TGT, V_PLAIN>, dp, st);
    GEMM_TRY(hipGetLastError());

    const uint32_t n_total = r.n_burnin + r.n_keep;
    const uint32_t L = r.n_leap;
    // the launches of ONE draw
    auto enqueue_draw = [&](hipStream_t s) -> int {
        const dim3 normals_grid((unsigned)(l.Cp / 256 + (l.Cp % 256 ? 1 : 0)), l.dK / 2);
        hipLaunchKernelGGL(dm ? gemm_normals_kernel<V_DENSE_M> : (box && !hmc) ? gemm_normals_kernel<V_BOX> : gemm_normals_kernel<V_PLAIN>, normals_grid, dim3(256), 0, s, dp);
        DrawParams pp = dp;
        if (dm && hmc) {                                               // L + 3 products with the mass matrices next to the L gradients
            if (int e = mass_product(A_lc, ev[0], EP_PRODUCT, nullptr, nullptr, pm, nullptr, nullptr, s)) return e;            // p = Lc z (:158)
            if (int e = mass_product(A_minv, pm, EP_PRODUCT, nullptr, nullptr, ev[1], nullptr, nullptr, s)) return e;          // Minv p (:160)
            per_chain(gemm_pre_kernel<V_DENSE_M>, dp, s);
            for (uint32_t k = 0; k < L; ++k) {
                if (int e = mass_product(A_minv, pm, EP_DRIFT, k == 0 ? th : thw[0], thw[0], nullptr, nullptr, nullptr, s)) return e;      // the drift (:171), in place from the second step on
                if (int e = evaluate(thw[0], (k + 1 < L) ? EP_KICKS : EP_LAST, nullptr, gprop, s)) return e;                  // the half-kick(s) (:175, :126)
            }
            if (int e = mass_product(A_minv, pm, EP_PRODUCT, nullptr, nullptr, ev[1], nullptr, nullptr, s)) return e;          // Minv p (:184)
            per_chain(gemm_post_kernel<GEMM_HMC, TGT, V_DENSE_M>, pp, s);
        } else if (dm) {                                               // mala: 5 products with the mass matrices next to the gradient
            if (int e = mass_product(A_m, gacc, EP_PRODUCT, nullptr, nullptr, ev[1], nullptr, nullptr, s)) return e;           // t = M g at the accepted state (mala.cpp:123)
            if (int e = mass_product(A_lc, ev[0], EP_MALA_PROPOSE, th, thw[0], ev[2], ev[1], nullptr, s)) return e;           // mean, proposal = mean + eps (Lc z) (:159)
            if (int e = evaluate(thw[0], EP_GRAD, nullptr, gprop, s)) return e;
            if (int e = mass_product(A_m, gprop, EP_MALA_REVERSE, thw[0], pm, ev[3], th, ev[2], s)) return e;                 // xa = prev - mean(prop), xb = prop - mean(prev)
            if (int e = mass_product(A_sinv, ev[3], EP_PRODUCT, nullptr, nullptr, ev[0], nullptr, nullptr, s)) return e;       // INV(Sigma) xa
            if (int e = mass_product(A_sinv, pm, EP_PRODUCT, nullptr, nullptr, ev[1], nullptr, nullptr, s)) return e;          // INV(Sigma) xb
            per_chain(gemm_post_kernel<GEMM_MALA, TGT, V_DENSE_M>, pp, s);
        } else if (hmc) {                                              // identity / diagonal precond_mat; with bounds the same launches, every one the bounded variant
            per_chain(box ? gemm_pre_kernel<V_BOX> : gemm_pre_kernel<V_PLAIN>, dp, s);
            for (uint32_t k = 0; k < L; ++k) {
                const uint32_t cur = k & 1u, nxt = cur ^ 1u;
                const bool last = k + 1 == L;
                if (int e = box ? evaluate(xw[cur], last ? EP_BOX_LAST : EP_BOX_LEAP, thw[nxt], gprop, s, thw[cur], xw[nxt])
                                : evaluate(thw[cur], last ? EP_LAST : EP_LEAP, thw[nxt], gprop, s)) return e;
            }
            pp.thw = thw[(L - 1u) & 1u]; pp.bx.xw = xw[(L - 1u) & 1u];
            per_chain(box ? gemm_post_kernel<GEMM_HMC, TGT, V_BOX> : gemm_post_kernel<GEMM_HMC, TGT>, pp, s);
        } else {                                                       // mala, rwmh (with bounds: evaluated at x)
            if (int e = evaluate(box ? xw[0] : thw[0], EP_GRAD, nullptr, gprop, s)) return e;
            per_chain(box ? gemm_post_kernel<GEMM_RWMH, TGT, V_BOX> : r.algo == GEMM_MALA ? gemm_post_kernel<GEMM_MALA, TGT> : gemm_post_kernel<GEMM_RWMH, TGT>, pp, s);
        }
        hipLaunchKernelGGL(gemm_advance_kernel, dim3(1), dim3(1), 0, s, w.draw_ctr);
        return (int)hipGetLastError();
    };

    // one draw's launches captured once, replayed n_total times (the draw index is device memory; every pointer is the same in every draw)
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    const bool graphed = r.use_graph && n_total > 1 && capture_and_instantiate(enqueue_draw, &graph, &exec);
    int rc = 0;
    for (uint32_t t = 0; t < n_total && rc == 0; ++t) rc = graphed ? (int)hipGraphLaunch(exec, st) : enqueue_draw(st);
    if (graphed) { const int e = release_graph(st, graph, exec); if (rc == 0) rc = e; }
    if (rc) return rc;

    DrawParams sp_out = dp;
    if (box) sp_out.th = w.xacc;                                       // the final state leaves through inv_transform too: a continued call transforms it again, as the literal kernel does
    hipLaunchKernelGGL(gemm_store_kernel, dim3(stride_grid((size_t)r.d * r.C)), dim3(256), 0, st, sp_out);
    GEMM_TRY(hipGetLastError());
    if (kernel_name) {
        static thread_local char name[112];
        snprintf(name, sizeof(name), "gemm_step_kernel<%d, %d> (%s%s%s)", hmc ? (L > 1 ? (dm ? EP_KICKS : box ? EP_BOX_LEAP : EP_LEAP) : box ? EP_BOX_LAST : EP_LAST) : EP_GRAD, TGT,
                 hmc ? "hmc" : r.algo == GEMM_MALA ? "mala" : "rwmh", graphed ? ", graph" : "", box ? ", bounds" : "");
        if (r.diag_mass || dm) { const size_t n = strlen(name); snprintf(name + n - 1, sizeof(name) - n + 1, dm ? ", dense precond_mat)" : ", diagonal precond_mat)"); }
        *kernel_name = name;
    }
    return 0;
}

int gemm_run(const GemmRun& r, hipStream_t st, const char** kernel_name)
{
    return r.X != nullptr ? gemm_run_t<TGT_LOGISTIC>(r, st, kernel_name) : gemm_run_t<TGT_DENSE>(r, st, kernel_name);
}

#include "gemm_nuts.hpp"          // mcmc::nuts on this route: per-chain trees, one product per tick for all chains

}  // namespace gemm
}  // namespace mi
