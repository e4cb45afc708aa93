// launch.h -- what the host side of every kernel launch shares (host code only): the opt-in to more than 64 KiB of dynamic LDS,
// the CU count of the current device, and the pointer-and-stride alignment check of the vectorised tensor accesses.
// A process may drive several devices: both caches are keyed by device and safe to use from several host threads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

// Dynamic LDS above the 64 KiB default needs hipFuncAttributeMaxDynamicSharedMemorySize, which is per device: set once per
// (kernel, device).  false = the runtime refused (nothing is remembered then: the next launch asks again).
template <class K>
inline bool dvla_allow_lds(K* kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return true;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  const std::pair<const void*, int> key(reinterpret_cast<const void*>(kernel), dev);
  std::lock_guard<std::mutex> lock(mu);
  if (done.count(key)) return true;
  if (hipFuncSetAttribute(key.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
  done.insert(key);
  return true;
}

// CU count of the current device; 0 = the query failed (callers choose their own fallback)
inline int dvla_num_cus() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
  static std::mutex mu;
  static std::vector<int> cus;
  std::lock_guard<std::mutex> lock(mu);
  if ((size_t)dev >= cus.size()) cus.resize(dev + 1, 0);
  if (cus[dev] <= 0 && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus[dev] = 0;
  return cus[dev];
}

// a bf16 tensor that `bytes`-wide (8 or 16) vector accesses may address: base pointer and the three element strides
inline bool dvla_aligned(const void* ptr, int64_t s0, int64_t s1, int64_t s2, int bytes) {
  const int elems = bytes / 2;
  return reinterpret_cast<uintptr_t>(ptr) % bytes == 0 && s0 % elems == 0 && s1 % elems == 0 && s2 % elems == 0;
}
