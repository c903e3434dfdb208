// linalg_stage.hpp -- the one number the device INV / CHOL_LOWER (linalg_device.hip) and their host-side routing (host_linalg.hpp) share: the LDS the
// kernels may stage their scaled pivot rows (INV: 2 d doubles) resp. finished column (CHOL_LOWER: d doubles) in.  d <= 3840 resp. 7680.
#pragma once

#include <cstddef>

constexpr size_t LINALG_STAGE_BYTES = 60 * 1024;
