// draws_bridge.hpp -- interface of the bridge-sampling kernels (draws_bridge.hip; the C entries are mi_mcmc_bridge_proposal, mi_mcmc_bridge_estimate and
// mi_mcmc_draws_bridge in draws_api.hip, where the stream's cached workspace lives).  Three pieces, every one with the ONE order include/mi_mcmc.h states:
//   propose_run   y = mu + L z of a group of proposal columns, z the Philox normals of STREAM_BRIDGE generated on the way into LDS, L z on the matrix cores
//   logg_run      the Gaussian log-density of every column of a slab: the DENSE log-kernel of the column centred on the way into LDS, minus ldh
//   the folds     l = logp - logg, a / b = exp(l - l*), SUMP's pieces of one iteration, and the terms' chunk sums for the error moments
// The plans decide time and memory only, never a bit of the result.
#pragma once

#include "draws_product.hpp"

namespace mi {
namespace dbridge {

using dprod::TM;
using dprod::TN;
using dprod::TK;
constexpr uint64_t BRIDGE_MAX_D = 65536;
constexpr uint64_t BRIDGE_PIECE = 16384;                  // values of one piece of SUMP (draws_psis.hpp: PSIS_BODY_PIECE)
constexpr uint64_t BRIDGE_CHUNK = 2048;                   // values of one chunk of the moments (draws_waic.hpp: WAIC_CHUNK)
constexpr uint64_t BRIDGE_PROP_BYTES = 2ull << 30;        // the budget of one group of proposal columns
constexpr size_t BRIDGE_LDS_BYTES = (size_t)2 * dprod::STAGE * sizeof(double);

// A d x d matrix packed as draws_product.hpp states: At [Kp][ldA], Kp = 16 ceil(d / 16), ldA = 128 ceil(d / 128)
struct MatPlan {
    uint64_t d = 0, Kp = 0, ldA = 0, n_row_tiles = 0, pack_grid = 0;
    size_t pack_bytes = 0;
};
MatPlan mat_plan(uint64_t d);
// the columns of one group under `budget` bytes (0, or more than BRIDGE_PROP_BYTES = BRIDGE_PROP_BYTES): a multiple of 128 -- below 128 a multiple of 16, the column
// tile of the matrix instruction, and never fewer than 16 --, at most N2
uint64_t group_cols(uint64_t d, uint64_t N2, uint64_t budget);

// Every function enqueues on `st` and returns a hipError_t as int (0 = enqueued); every pointer is device memory.
// M (row-major d x d) -> At (mat_plan(d).pack_bytes)
int pack_run(const MatPlan& p, const double* M, double* At, hipStream_t st);
// y[a * ldy + k] = mu[a] + (L z^(col0 + k))_a for k < ncols, a < d: At_L the packed L (its upper triangle zero)
int propose_run(const MatPlan& p, const double* At_L, const double* mu, uint64_t seed, uint64_t col0, uint64_t ncols, uint64_t ldy, double* y, hipStream_t st);
// out[k] = (-0.5 * dot4(e, Pg e)) - ldh of the K = n_keep * C columns of the slab x [n_keep][d][C], e = x - mu: At_P the packed Pg
int logg_run(const MatPlan& p, const double* At_P, const double* mu, double ldh, const double* x, uint64_t n_keep, uint64_t C, double* out, hipStream_t st);
// out[k] = a[k] - b[k]
int diff_run(const double* a, const double* b, uint64_t n, double* out, hipStream_t st);
// v[k] = exp(v[k] - lstar), in place
int exp_shift_run(double* v, uint64_t n, double lstar, hipStream_t st);
// part[p] = SUM(piece p) of f1 = a / (s1 a + s2 r) over a [N2], p < ceil(N2 / 16384); then of f2 = 1 / (s1 b + s2 r) over b [N1]
int pieces_run(const double* a, uint64_t N2, const double* b, uint64_t N1, double s1, double s2, double r, double* part, hipStream_t st);
// chunk c of f1 (then of f2): stat[3 c .. 3 c + 2] = (shift, S1, S2) of mi_mcmc_draws_waic's ORDER; f2_out (may be NULL) [N1] <- f2
int moments_run(const double* a, uint64_t N2, const double* b, uint64_t N1, double s1, double s2, double r, double* stat, double* f2_out, hipStream_t st);
// v[k] = NaN
int fill_nan_run(double* v, uint64_t n, hipStream_t st);

inline uint64_t n_pieces(uint64_t n) { return (n + BRIDGE_PIECE - 1) / BRIDGE_PIECE; }
inline uint64_t n_chunks(uint64_t n) { return (n + BRIDGE_CHUNK - 1) / BRIDGE_CHUNK; }

}  // namespace dbridge
}  // namespace mi
