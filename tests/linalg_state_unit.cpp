// One of two host translation units over mcmc_amd/csrc/host_linalg.hpp (tests/test_linalg_state_cpu.py compiles this file twice, -DUNIT=a and
// -DUNIT=b, into one shared library): each exports what ITS copy of the header's inline functions sees.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../mcmc_amd/csrc/host_linalg.hpp"

#define CAT2(a, b) a##b
#define CAT(a, b) CAT2(a, b)
#define FN(name) CAT(CAT(unit_, UNIT), CAT(_, name))

// stands for the device CHOL_LOWER the product installs; the test never lets a factorisation reach it
static int installed_cholesky_lower(const double*, size_t, double*) { return -1; }

extern "C" {
const void* FN(accel)(void) { return &linalg_accel(); }
uint64_t FN(n_computed)(void) { return linalg_accel().n_computed.load(std::memory_order_relaxed); }
int FN(cholesky_lower)(const double* A, uint32_t d, double* L)
{
    std::vector<double> v;
    const int rc = host_cholesky_lower(A, d, v);
    if (rc == 0) std::memcpy(L, v.data(), (size_t)d * d * sizeof(double));
    return rc;
}
void FN(install)(void) { linalg_accel().cholesky_lower = installed_cholesky_lower; }
void FN(uninstall)(void) { linalg_accel().cholesky_lower = nullptr; }
void FN(set_stage_bytes)(uint32_t bytes) { linalg_set_stage_bytes(bytes); }
int FN(on_device)(int which, uint32_t d) { return linalg_on_device(which, d) ? 1 : 0; }
}
