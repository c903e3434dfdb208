// de_launch.hip -- translation unit of the mcmc::de kernels (de.hpp)
#include "de.hpp"
#include "launchers.hpp"
#include "launch_common.hpp"

namespace mi {
namespace {

template <int NT, bool GENERAL>
int gauss(const DeParams& prm, hipStream_t st)
{
    const size_t lds = (size_t)NT * 4 * NT * 64 * sizeof(double) + (GENERAL ? (size_t)16 * NT * (2 * sizeof(double) + sizeof(int)) : 0);
    auto kern = de_gauss_mfma_kernel<NT, GENERAL>;
    note_kernel("de_gauss_mfma_kernel<%d, %s>", NT, GENERAL ? "true" : "false");
    MI_LAUNCH_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)((prm.NP + 63) / 64)), dim3(256), lds, st, prm);
    return (int)hipGetLastError();
}

}  // namespace

int launch_de_gauss(const DeParams& prm, int nt, bool general, hipStream_t st)
{
    if (general) return MI_DISPATCH_NT(nt, (gauss<1, true>(prm, st)), (gauss<2, true>(prm, st)), (gauss<4, true>(prm, st)), (gauss<8, true>(prm, st)));
    return MI_DISPATCH_NT(nt, (gauss<1, false>(prm, st)), (gauss<2, false>(prm, st)), (gauss<4, false>(prm, st)), (gauss<8, false>(prm, st)));
}

int launch_de_literal(const DeParams& prm, unsigned n_wg, hipStream_t st)
{
    if (n_wg == 0) return 0;
    note_kernel("de_literal_kernel");
    hipLaunchKernelGGL(de_literal_kernel, dim3(n_wg), dim3(256), 0, st, prm);
    return (int)hipGetLastError();
}

}  // namespace mi
