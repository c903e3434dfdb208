// probes_kc2.hip -- the math and normals probes of probes.hip once more, with det_math.hpp built as logistic_lds.hip, logistic_nuts.hip and
// logistic_nuts_dense_m.hip build it: every polynomial coefficient assembled from two 32-bit literals at its point of use, rng_normal_pair out of line.
#define MI_KC_MODE 2
#define MI_RNG_NOINLINE 1
#include <hip/hip_runtime.h>

#include "host_common.hpp"
#include "mi_mcmc_probes.h"
#include "det_math.hpp"
#include "probe_kernels.hpp"

extern "C" {

int mi_probe_math_kc2(int fn, const double* x, uint64_t n, double* out, double* out2) { return mi::probe::run_math<MI_KC_MODE>(fn, x, n, out, out2); }

int mi_probe_math2_kc2(int fn, const double* x, const double* y, uint64_t n, double* out) { return mi::probe::run_math2<MI_KC_MODE>(fn, x, y, n, out); }

int mi_probe_normals_kc2(int variant, uint64_t seed, uint64_t chain, uint32_t draw, uint32_t stream, uint64_t d, double* out)
{
    return mi::probe::run_normals<MI_KC_MODE>(variant, seed, chain, draw, stream, d, out);
}

}  // extern "C"
