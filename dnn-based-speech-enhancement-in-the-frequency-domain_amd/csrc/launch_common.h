// Host-side helpers shared by the launchers of the conv GEMM kernel families (rungemm.hip asks each family's `choose` in order and hands the
// KernelChoice to its `launch`): the device's CU count, a kernel's resident workgroups per CU, and the knob-driven rule of the families with a
// persistent grid.  No knob is read or kept here: the families read theirs by name on every launch (tuning.h).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <climits>
#include "dev_common.h"

namespace sefd {

// The kernels a form table points to all take the descriptor and the arena bases by value
using GemmKernel = void (*)(const RunGemm, const ArenaBases);

// Compute units of the current device, 256 without one (plan inspection on the host).  Asked once per process.
inline int device_cus() {
  static const int ncu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
      (void)hipGetLastError();
      return 256;
    }
    return n;
  }();
  return ncu;
}

// Resident workgroups per CU of `kern` at `threads` threads from the occupancy query, never more than `cap`; without a device: `fallback`.
// Asked once per process and kernel: `slot` is the cache of the kernel's row in its form table (0: not asked yet).
inline int resident_wgs_per_cu(std::atomic<int>& slot, GemmKernel kern, int threads, int fallback, int cap = INT_MAX) {
  int n = slot.load(std::memory_order_relaxed);
  if (n != 0) return n;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(kern), threads, 0) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    n = fallback;
  } else if (n > cap) {
    n = cap;
  }
  slot.store(n, std::memory_order_relaxed);
  return n;
}

// The rule of a family with a persistent grid and the knobs KNOB / KNOB_GRID, which the family reads by name on every launch.  mode = KNOB: 0 off,
// 1 (unset) the family's default rule, 2 every launch of its forms (what the default rule is stays with the family).  forced = KNOB_GRID: 0 the resident
// workgroups, any other value that grid (the tests walk all work units with 1 and 3 workgroups).  The grid is capped by the work units and is at least 1.
inline bool knob_takes(int mode, bool by_default) { return mode > 0 && (mode == 2 || by_default); }
inline int64_t knob_grid(int64_t forced, int wgs_per_cu) { return forced > 0 ? forced : (int64_t)wgs_per_cu * device_cus(); }
inline int cap_grid(int64_t grid, int64_t units) {
  if (grid > units) grid = units;
  return (int)(grid < 1 ? 1 : grid);
}

}  // namespace sefd
