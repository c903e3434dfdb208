// aees_launch.hip -- translation unit of the mcmc::aees kernel (aees.hpp)
#include "aees.hpp"
#include "launchers.hpp"
#include "launch_common.hpp"

namespace mi {

int launch_aees_literal(const AeesParams& prm, unsigned n_wg, hipStream_t st)
{
    if (n_wg == 0) return 0;
    note_kernel("aees_literal_kernel");
    hipLaunchKernelGGL(aees_literal_kernel, dim3(n_wg), dim3(256), 0, st, prm);
    return (int)hipGetLastError();
}

}  // namespace mi
