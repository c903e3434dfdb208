// nuts_points.hpp -- the geometry of the memoised NUTS trajectory, shared by the kernels that evaluate a doubling point by point (nuts_lds.hpp, gemm_nuts.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace mi {
namespace lds_nuts {
// The memoised trajectory (nuts_memo.hpp, DESIGN.md 4.4e: leaf i of a doubling is the state LF^{n(i)}(prev_draw, mntm_vec), n(i) = 1 + the sum over the set
// bits k of i of (k + 1); the U-turn test of a level-l node whose first leaf sits at point n1 compares the points n1 and n1 + l).
// point of leaf i
__host__ __device__ constexpr uint32_t npt_of(uint32_t i)
{
    uint32_t n = 1;
    for (uint32_t k = 0; k < 10; ++k) if ((i >> k) & 1u) n += k + 1;
    return n;
}
// is there a level-l node in a doubling of depth j whose first leaf sits at point n1?  (n1 - 1 must be a sum of distinct integers of {l + 1 .. j})
__host__ __device__ constexpr bool pair_used(int l, int n1, int j)
{
    const int m = n1 - 1;
    for (int t = 0; t <= j - l; ++t) {
        const int lo = t * (l + 1) + t * (t - 1) / 2, hi = t * j - t * (t - 1) / 2;
        if (m >= lo && m <= hi) return true;
    }
    return false;
}
// bit l of [j][m]: point m of a depth-j doubling closes a level-l test (against point m - l)
struct PmTable { uint16_t v[10][48]; };
constexpr PmTable make_pm_table()
{
    PmTable t{};
    for (int j = 0; j < 10; ++j)
        for (int m = 0; m < 48; ++m) {
            uint32_t bits = 0;
            for (int l = 1; l <= j; ++l)
                if (m - l >= 1 && pair_used(l, m - l, j)) bits |= 1u << l;
            t.v[j][m] = (uint16_t)bits;
        }
    return t;
}
__device__ const PmTable pm_table = make_pm_table();
// npt_of on the device: 1 + popc(i) + sum_b 2^b popc(i & M_b), M_b = the bit positions k with bit b of k set
__device__ __forceinline__ uint32_t npt_of_dev(uint32_t i)
{
    return 1u + (uint32_t)__builtin_popcount(i) + (uint32_t)__builtin_popcount(i & 0x2AAu) + 2u * (uint32_t)__builtin_popcount(i & 0xCCu)
         + 4u * (uint32_t)__builtin_popcount(i & 0xF0u) + 8u * (uint32_t)__builtin_popcount(i & 0x300u);
}
}  // namespace lds_nuts
}  // namespace mi
