// kit4b_amd/csrc/k4_pe_insert_rule.h -- the two rules of kalign's per-target PE insert table (`-3`) that are worth stating once, for
// the kernels of k4_peinserts.hip and for the host (k4_pe_insert_bin_host, k4_pe_insert_median_host):
//   k4_pei_bin     <- the column of an insert length, CKAligner::ReportPEInsertLenDist  ngskit4b/KAligner.cpp:5420-5428
//   k4_pei_median  <- CKAligner::MedianInsertLen :5256-5319, from the target's SORTED insert lengths and its first one in walk order
//
// MedianInsertLen is not the textbook median.  With f(v) = count(< v) - count(> v) over all n values: it takes Lo = min, Hi = max,
// then walks elements 1 .. n-1 (element 0 is never a candidate), passes over a candidate outside [Lo, Hi], returns a candidate with
// f = 0, and otherwise moves Lo (f < 0) or Hi (f > 0) to the candidate; at the end (Lo + Hi) / 2 in 32 bits.
// f rises strictly from one distinct value to the next, f(min) < 0 < f(max) when min < max, so at most one value v* balances, every
// value Lo moves to has f < 0 and every value Hi moves to f > 0: v* always lies inside (Lo, Hi) and is returned where it is met, and
// without it Lo ends on the largest candidate with f < 0 (or stays min), Hi on the smallest with f > 0 (or stays max).  Hence the
// result depends on the order of the values only through element 0: a value that occurs once, as element 0, is no candidate.
// The sorted middle element s[n / 2] is v*, or the value next to the sign change of f: one step to the neighbouring distinct value
// finds the other side.  (The reference's min / max scan takes 0 for "not set yet"; an insert length is never 0, and neither rule is
// claimed for arrays that hold one.)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define K4_PEI_BINS 52           // "<100", 100, 110 .. 590, ">600"
#define K4_PEI_MAX_PAIRS 1000000u  // only the first million pairs of a target are counted (:5352, :5404)

// 100..108 share "Insert 100bp", 109..118 "Insert 110bp", .., 599 and 600 land in the last column: the arithmetic is the reference's
__host__ __device__ inline uint32_t k4_pei_bin(uint32_t tlen) {
  if (tlen < 100u) return 0u;
  if (tlen > 600u) return 51u;
  return 1u + (tlen - 99u) / 10u;
}

// n ascending values, W words apart (the kernel reads them out of the low words of its sorted 64-bit keys: W = 2)
template <int W>
struct K4PeiSorted {
  const uint32_t* p;
  uint32_t n;
  __host__ __device__ uint32_t operator[](uint32_t i) const { return p[(size_t)W * i]; }
  // the first position that holds a value >= v (past = false) / > v (past = true)
  __host__ __device__ uint32_t bound(uint32_t v, bool past) const {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if ((*this)[mid] < v || (past && (*this)[mid] == v)) lo = mid + 1; else hi = mid;
    }
    return lo;
  }
};

// s: the kept insert lengths of a target, ascending; first: the one of its first pair in walk order
template <int W>
__host__ __device__ inline uint32_t k4_pei_median(const K4PeiSorted<W> s, uint32_t first) {
  const uint32_t n = s.n;
  if (n == 0) return 0u;
  if (n == 1) return s[0];
  if (n == 2) return (s[0] + s[1]) / 2u;
  const uint32_t mn = s[0], mx = s[n - 1];
  if (mn == mx) return mx;
  // p: the largest value with f < 0, q: the smallest with f > 0, around the middle element v (lb <= n / 2 < ub)
  const uint32_t v = s[n / 2];
  const uint32_t lb = s.bound(v, false), ub = s.bound(v, true);
  const int64_t f = (int64_t)lb + (int64_t)ub - (int64_t)n;
  uint32_t p_at, q_at;  // the first position of p, the first position of q
  if (f == 0) {
    if (ub - lb >= 2u || first != v) return v;  // v* is met as a candidate
    p_at = s.bound(s[lb - 1], false);           // v* is element 0 alone: its two neighbours are candidates
    q_at = ub;
    return (s[p_at] + s[q_at]) / 2u;
  }
  if (f > 0) { q_at = lb; p_at = s.bound(s[lb - 1], false); }
  else { p_at = lb; q_at = ub; }
  uint32_t p = s[p_at], q = s[q_at];
  // a bound that occurs once, as element 0, was never a candidate: the next distinct value outwards is (min and max are bounds anyway)
  if (p != mn && first == p && s.bound(p, true) - p_at == 1u) p = s[p_at - 1];
  if (q != mx && first == q && s.bound(q, true) - q_at == 1u) q = s[q_at + 1];
  return (p + q) / 2u;
}
