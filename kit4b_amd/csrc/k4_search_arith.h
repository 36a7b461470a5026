// kit4b_amd/csrc/k4_search_arith.h -- the index arithmetic the search-call families share (DESIGN.md "Search-call families: shared
// scaffold"): which table entry a locus belongs to, which run a candidate belongs to, which loci a launch takes.  Included by
// k4_device.h; it needs nothing of the device, so that a host program can hold it against a linear scan
// (tests/test_search_scaffold_cpu.py: K4_SA_FN emptied).
#pragma once
#include <stdint.h>

#ifndef K4_SA_FN
#define K4_SA_FN __device__ __forceinline__
#endif

// The last i in [0, n) with at(i) <= key, for at() ascending (equal neighbours are empty runs: the last of them answers), n >= 1
// and at(0) <= key: the entry, span or run that holds a locus when at(i) is the number of loci in front of i.
template <typename I, typename K, typename At>
K4_SA_FN I k4d_last_le(I n, K key, At at) {
  I lo = 0, hi = n - 1;
  while (lo < hi) {
    const I mid = (lo + hi + 1) >> 1;
    if (at(mid) <= key) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// candidate g (below the total) of a runs layout (k4d_runs_layout, k4_device.h) is occurrence occ of run item, the last run in
// 0 .. hi whose candidates start at or before g; any hi at or behind the last run that has a candidate gives the same answer, the
// entries behind that run holding the total
K4_SA_FN void k4d_runs_locate(uint32_t g, uint32_t hi, const uint32_t* g_pre, uint32_t& item, uint32_t& occ) {
  item = k4d_last_le(hi + 1u, g, [&](uint32_t i) { return g_pre[i]; });
  occ = g - g_pre[item];
}

// [0, total) in windows of at most per_launch, ascending: fn(k0, k1) per window, none for total 0.  A family that gives every
// locus a wave launches one grid per window, so that a grid stays below the limit it chose (host side only).
template <typename F>
inline void k4s_launch_windows(uint64_t total, uint64_t per_launch, F fn) {
  for (uint64_t k0 = 0; k0 < total; k0 += per_launch) fn(k0, total - k0 < per_launch ? total : k0 + per_launch);
}
