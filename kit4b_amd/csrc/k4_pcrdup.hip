// kit4b_amd/csrc/k4_pcrdup.hip -- `kalign -k <WinLen>`: PCR differential-amplification artefact reduction on the device, over
// the SE records k4_kalign_*_batch_dev (and the stages behind it) left in HBM:
//   k4_reduce_pcr_dups_dev  <- CKAligner::ReducePCRduplicates  ngskit4b/KAligner.cpp:2303-2400
//                              CKAligner::NumUpUniques / NumDnUniques  :10714-10830
//
// The reference walks the accepted reads in SortHitMatch order (chrom, AdjStartLoci, AdjHitLen, strand, LowMMCnt; ties in load
// order).  From each read it counts the distinct same-strand start sites within WinLen up- and downstream, buckets the larger
// count into LimitDups, keeps that many of the following reads of the same (chrom, start, length, strand) and marks the rest
// eNARPCRdup; it resumes behind the last read it marked.  No walk marks its own head, so every (chrom, strand, start) that has
// an accepted read keeps one: the window counts do not depend on the marking, they are the same for every read of a site, and
// the walk marks exactly the reads whose rank within their (chrom, start, length, strand) run exceeds the run's LimitDups
// (a run whose surplus is within the limit is walked again from its next read, with the same limit, and keeps everything).
// Hence, data-parallel:
//   1. select the accepted reads; sort them by (chrom, strand, start) and then (length, low_mm), stable over load order
//   2. one scan numbers the distinct (chrom, strand, start) sites and finds each read's run head
//   3. per site: two binary searches over the sorted site list give the up- / downstream counts -> LimitDups
//   4. per read: rank within the run > LimitDups -> NAR 9 (DP), NumHits = LowHitInstances = 0
// DESIGN.md "PCR duplicate reduction" has the argument in full.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <rocprim/rocprim.hpp>
#include "k4_device.h"
#include "k4_stage.h"

namespace {

struct IsUniqueAccepted {  // the reads the walk looks at: accepted, one hit (SE: every accepted read before -x / -r5)
  const k4_read_result* rr;
  __device__ bool operator()(uint32_t i) const { return rr[i].nar == K4_NAR_ACCEPTED && rr[i].num_hits == 1; }
};

// major key: chrom (bits 33..), strand (bit 32: '-' after '+'), AdjStartLoci (bits 0..31)
__device__ __forceinline__ uint64_t site_key(const k4_hit& h) {
  return ((uint64_t)h.chrom_id << 33) | ((uint64_t)(h.strand == '-') << 32) | k4d_adj_start(h);
}

__global__ void __launch_bounds__(256) k4k_pcr_minor_keys(uint32_t m, const uint32_t* __restrict__ idx, const k4_read_result* __restrict__ rr,
                                                          const k4_hit* __restrict__ hits, int max_ml, uint32_t* __restrict__ minor) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  const uint32_t i = idx[j];
  const int32_t mm = rr[i].low_mm;
  minor[j] = (k4d_adj_len(hits[(int64_t)i * max_ml]) << 16) | (uint32_t)min(max(mm, 0), 0xFFFF);
}

__global__ void __launch_bounds__(256) k4k_pcr_major_keys(uint32_t m, const uint32_t* __restrict__ idx, const k4_hit* __restrict__ hits, int max_ml,
                                                          uint64_t* __restrict__ major) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  major[j] = site_key(hits[(int64_t)idx[j] * max_ml]);
}

// scan element: sites seen so far (inclusive) and the position of the current run's head
struct SiteRun {
  uint32_t site, head;
};
struct SiteRunOp {
  __device__ SiteRun operator()(const SiteRun& a, const SiteRun& b) const { return {a.site + b.site, a.head > b.head ? a.head : b.head}; }
};

__global__ void __launch_bounds__(256) k4k_pcr_heads(uint32_t m, const uint32_t* __restrict__ order, const uint64_t* __restrict__ major,
                                                     const k4_hit* __restrict__ hits, int max_ml, SiteRun* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  bool site = j == 0, run = j == 0;
  if (j) {
    site = major[j] != major[j - 1];
    run = site || k4d_adj_len(hits[(int64_t)order[j] * max_ml]) != k4d_adj_len(hits[(int64_t)order[j - 1] * max_ml]);
  }
  out[j] = {site ? 1u : 0u, run ? j : 0u};
}

__global__ void __launch_bounds__(256) k4k_pcr_sites(uint32_t m, const uint64_t* __restrict__ major, const SiteRun* __restrict__ sr,
                                                     uint64_t* __restrict__ sites) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  if (j == 0 || major[j] != major[j - 1]) sites[sr[j].site - 1] = major[j];
}

// first position in sites[lo, hi) whose key is >= (upper: >) `key`
__device__ __forceinline__ uint32_t bound(const uint64_t* __restrict__ sites, uint32_t lo, uint32_t hi, uint64_t key, bool upper) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint64_t v = sites[mid];
    if (upper ? v <= key : v < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// LimitDups of one site (KAligner.cpp:2330-2356).  NumUpUniques counts the distinct starts in [start - WinLen, start) -- no lower
// bound while start <= WinLen, which for starts >= 0 is the same as a bound at 0; NumDnUniques those in (start, start + WinLen].
// Same chromosome and strand: the other fields of the key.
__global__ void __launch_bounds__(256) k4k_pcr_limits(const SiteRun* __restrict__ last, const uint64_t* __restrict__ sites, int win,
                                                      int32_t* __restrict__ lim) {
  const uint32_t n_sites = last->site;
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= n_sites) return;
  const uint64_t key = sites[q], cs = key & ~0xFFFFFFFFull;
  const uint32_t start = (uint32_t)key;
  const uint32_t lo = start > (uint32_t)win ? start - (uint32_t)win : 0u;
  const uint64_t hi = (uint64_t)start + (uint32_t)win;
  const uint32_t up = q - bound(sites, 0, q, cs | lo, false);
  const uint32_t dn = bound(sites, q + 1, n_sites, cs | (hi > 0xFFFFFFFFull ? 0xFFFFFFFFull : hi), true) - q - 1;
  const int limit_dups = (int)max(up, dn);
  const int prop = (int)(((double)limit_dups / win) * 100.0);
  lim[q] = prop < 5 ? 1 : prop <= 10 ? 2 : prop <= 20 ? 3 : prop <= 40 ? 4 : prop <= 60 ? 5 : prop <= 80 ? 10 : 50;
}

__global__ void __launch_bounds__(256) k4k_pcr_mark(uint32_t m, const uint32_t* __restrict__ order, const SiteRun* __restrict__ sr,
                                                    const int32_t* __restrict__ lim, k4_read_result* __restrict__ rr,
                                                    unsigned long long* __restrict__ n_marked) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  bool mark = false;
  if (j < m) {
    const SiteRun s = sr[j];
    const uint32_t limit = lim ? (uint32_t)lim[s.site - 1] : 0u;
    if (j - s.head > limit) {
      const uint32_t i = order[j];
      rr[i].nar = K4_NAR_PCRDUP;
      rr[i].num_hits = 0;
      rr[i].inst = 0;
      mark = true;
    }
  }
  const int c = __syncthreads_count(mark);
  if (threadIdx.x == 0 && c) atomicAdd(n_marked, (unsigned long long)c);
}

}  // namespace

extern "C" int k4_reduce_pcr_dups_dev(k4_index* ix, int32_t win_len, int64_t n_reads, int32_t max_ml, void* d_rr, void* d_hits,
                                      int64_t* n_dups, void* stream) {
  if (!ix) return K4_ERR_PARAMS;
  if (n_dups) *n_dups = 0;
  if (win_len < 0 || win_len > 250) return k4_fail(ix, K4_ERR_PARAMS, "PCR artefact window length %d outside of range 0..250", (int)win_len);
  if (n_reads <= 0) return K4_OK;
  if (!d_rr || !d_hits || max_ml < 1) return k4_fail(ix, K4_ERR_PARAMS, "null buffer");
  if (n_reads >= 0xFFFFFF00ll) return k4_fail(ix, K4_ERR_PARAMS, "at most 2^32-256 reads per call");
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  const k4_read_result* rr = (const k4_read_result*)d_rr;
  const k4_hit* hits = (const k4_hit*)d_hits;
  K4DevBuf idx0, idx1, cnt;
  K4_HIP(ix, cnt.alloc(8));
  K4_HIP(ix, hipMemsetAsync(cnt.p, 0, 8, st));
  uint64_t m64 = 0;  // the accepted reads, in load order
  K4_TRY(k4s_select_indices(ix, idx0, (size_t)n_reads, IsUniqueAccepted{rr}, st, &m64));
  if (m64 < 2) return K4_OK;  // a lone read is the head of its run
  const uint32_t m = (uint32_t)m64;
  const unsigned nb = (m + 255u) / 256u;
  K4DevBuf mk0, mk1, kk0, kk1, sr, srs, sites, lim;
  K4_HIP(ix, idx1.alloc((size_t)m * 4));
  K4_HIP(ix, mk0.alloc((size_t)m * 4));
  K4_HIP(ix, mk1.alloc((size_t)m * 4));
  K4_HIP(ix, kk0.alloc((size_t)m * 8));
  K4_HIP(ix, kk1.alloc((size_t)m * 8));
  // 1. two stable LSD radix sorts over load order: (length, low_mm) first, then (chrom, strand, start)
  hipLaunchKernelGGL(k4k_pcr_minor_keys, dim3(nb), dim3(256), 0, st, m, idx0.as<uint32_t>(), rr, hits, (int)max_ml, mk0.as<uint32_t>());
  K4_HIP(ix, hipGetLastError());
  rocprim::double_buffer<uint32_t> mk(mk0.as<uint32_t>(), mk1.as<uint32_t>());
  rocprim::double_buffer<uint32_t> vb(idx0.as<uint32_t>(), idx1.as<uint32_t>());
  K4_TRY(k4s_sort_pairs<K4DevBuf>(ix, mk, vb, (size_t)m, 0u, 32u, st));
  hipLaunchKernelGGL(k4k_pcr_major_keys, dim3(nb), dim3(256), 0, st, m, vb.current(), hits, (int)max_ml, kk0.as<uint64_t>());
  K4_HIP(ix, hipGetLastError());
  rocprim::double_buffer<uint64_t> kk(kk0.as<uint64_t>(), kk1.as<uint64_t>());
  K4_TRY(k4s_sort_pairs<K4DevBuf>(ix, kk, vb, (size_t)m, 0u, 64u, st));  // (chrom ids are the index's EntryIDs: any 32-bit value)
  const uint32_t* order = vb.current();
  const uint64_t* major = kk.current();
  // 2. site numbers and run heads
  K4_HIP(ix, sr.alloc((size_t)m * sizeof(SiteRun)));
  K4_HIP(ix, srs.alloc((size_t)m * sizeof(SiteRun)));
  hipLaunchKernelGGL(k4k_pcr_heads, dim3(nb), dim3(256), 0, st, m, order, major, hits, (int)max_ml, sr.as<SiteRun>());
  K4_HIP(ix, hipGetLastError());
  K4_TRY(k4s_inclusive_scan<K4DevBuf>(ix, sr.as<SiteRun>(), srs.as<SiteRun>(), (size_t)m, SiteRunOp(), st));
  // 3. LimitDups per site (WinLen 0: LimitDups 0 everywhere)
  const int32_t* d_lim = nullptr;
  if (win_len > 0) {
    K4_HIP(ix, sites.alloc((size_t)m * 8));
    K4_HIP(ix, lim.alloc((size_t)m * 4));
    hipLaunchKernelGGL(k4k_pcr_sites, dim3(nb), dim3(256), 0, st, m, major, srs.as<SiteRun>(), sites.as<uint64_t>());
    hipLaunchKernelGGL(k4k_pcr_limits, dim3(nb), dim3(256), 0, st, srs.as<SiteRun>() + (m - 1), sites.as<uint64_t>(), (int)win_len,
                       lim.as<int32_t>());
    K4_HIP(ix, hipGetLastError());
    d_lim = lim.as<int32_t>();
  }
  // 4. the reads ranked behind their run's limit
  hipLaunchKernelGGL(k4k_pcr_mark, dim3(nb), dim3(256), 0, st, m, order, srs.as<SiteRun>(), d_lim, (k4_read_result*)d_rr,
                     cnt.as<unsigned long long>());
  K4_HIP(ix, hipGetLastError());
  unsigned long long c = 0;
  K4_TRY(k4s_read_back(ix, &c, cnt.p, st));
  if (n_dups) *n_dups = (int64_t)c;
  return K4_OK;
}
