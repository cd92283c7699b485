// rt_wf_launch.hpp — how the wavefront pipeline's translation units
// (rt_wavefront.hip, rt_wavefront_glb.hip) launch a kernel: the grid from the
// kernel's occupancy, and the launch itself. Internal to those two files.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "rt_wf_device.hpp"

namespace rtamd {

// Blocks for n items: what the device holds at once at most (the kernels loop
// over gridDim x blockDim), one at least.
template <typename K>
static int occupancy_grid(K kern, int block, size_t lds, unsigned n) {
  int dev = 0, n_cu = 0, per_cu = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, block, lds) != hipSuccess || per_cu < 1) per_cu = 1;
  long long want = ((long long)n + block - 1) / block;
  long long cap = (long long)n_cu * per_cu;
  long long g = std::min(want, cap);
  return (int)std::max(g, 1LL);
}

// The deep Csg units' state buffer of the scene a launch passes (its first argument, where that is a
// DevScene) holds a lane for every thread of the grid: csg_deep_eval indexes it by the thread's number.
template <typename A, typename... Rest>
inline bool deep_state_holds(unsigned, unsigned, const A&, const Rest&...) { return true; }
template <typename... Rest>
inline bool deep_state_holds(unsigned grid, unsigned block, const DevScene& sc, const Rest&...) {
  return sc.csg_deep_levels <= 0 || (unsigned long long)grid * block <= sc.csg_deep_lanes;
}

// One launch over n items with `dyn` bytes of dynamic LDS: the kernel's limit
// raised to it, the occupancy grid, and the launch, carrying the profiling
// events e0 / e1 in the dispatch itself when given (no event packets between
// the kernels). Returns the launch's error.
template <typename K, typename... Args>
static hipError_t wf_launch(K kern, int block, size_t dyn, unsigned n, hipStream_t stream, hipEvent_t e0, hipEvent_t e1,
                            const Args&... args) {
  if (dyn > 0) WF_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  const dim3 grid(occupancy_grid(kern, block, dyn, n));
  // (a launch larger than the workspace's deep state is refused here, not answered wrongly on the device)
  if (!deep_state_holds(grid.x, (unsigned)block, args...)) return hipErrorInvalidValue;
  if (e0) hipExtLaunchKernelGGL(kern, grid, dim3(block), dyn, stream, e0, e1, 0, args...);
  else hipLaunchKernelGGL(kern, grid, dim3(block), dyn, stream, args...);
  return hipGetLastError();
}

}  // namespace rtamd
