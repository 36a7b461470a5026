// kit4b_amd/csrc/k4_siteprefs.hip -- `kalign -8 <file> [-9 <ofs>]`: the start-site octamer preferences, counted on the device over
// the records the align entry points and the global stages left in HBM, scaled and printed on the host:
//   k4_site_prefs_dev    <- the walk of CKAligner::ProcessSiteProbabilites  ngskit4b/KAligner.cpp:8750-8821
//   k4_write_site_prefs  <- its scale step :8823-8872 and CKAligner::WriteSitePrefs :8910-8945
//
// The reference walks the accepted reads in SortHitMatch order (chrom, AdjStartLoci, AdjHitLen, strand, mismatches; ties in load
// order here, as in the SAM body).  A two-segment read is passed over before anything else.  From the RAW Seg[0].MatchLoci /
// MatchLen it takes the octamer at `ofs` from the read's 5' end on the target, counts it per strand (NumOccs) and counts it once
// more (NumSites) when its locus differs from the one of the last read it counted on this sequence.  Hence, data-parallel:
//   1. select the accepted reads; two stable radix sorts (k4_stage.h) give the walk order
//   2. k4k_site_octamers, a lane per sorted read: the locus in the reference's 32-bit unsigned arithmetic (kept with its wrap and
//      clamp), the eight bases out of one 64-bit window of ref2, the exception data for N, reverse complement by bit operations
//   3. select the counted reads, in order: the reads the walk `continue`s over (two segments, an N in the octamer) leave PrevLoci
//      alone, so behind the compaction "differs from the last counted read's locus on this sequence" is a compare with the neighbour
//   4. the two tables of 2 x 65536 counters, in one of two forms (K4_SITEPREFS_HIST=atomic|sort chooses; DESIGN.md has both times):
//      k4k_site_hist_atomic  global atomics, the equal keys of a wave added once by their first lane
//      sort                  radix sort of (strand, octamer, head) + run lengths (rocprim::run_length_encode) + k4k_site_hist_runs
// A read whose signed locus lies in -8..-1 makes the reference read an uninitialised array; it is not counted here and leaves
// the carried locus alone (DESIGN.md lists it as an unpinned difference).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#include "k4_device.h"
#include "k4_stage.h"

#define K4_SITE_OCTS 65536u
#define K4_SITE_UNCOUNTED 0xFFFFFFFFu
#define K4_SITE_LEADERS 8  // equal-key groups a wave settles by ballot before its remaining lanes add one by one

namespace {

struct IsSiteRead {  // accepted (:8752); a two-segment read is sorted along and comes out uncounted
  K4ReadSet s;
  uint32_t n_entries;
  __device__ bool operator()(uint32_t i) const {
    k4_hit h;
    return s.accepted(i, h) && h.chrom_id >= 1 && h.chrom_id <= n_entries;
  }
};

// the formatter's keys (k4_io.hip): AdjHitLen, strand, mismatches; then chrom, AdjStartLoci
__global__ void __launch_bounds__(256) k4k_site_key_minor(const K4ReadSet s, uint32_t m, const uint32_t* __restrict__ idx, uint32_t* __restrict__ key) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  const k4_hit h = s.hit(idx[j]);
  key[j] = (k4d_adj_len(h) << 16) | ((uint32_t)h.strand << 8) | h.mismatches;
}
__global__ void __launch_bounds__(256) k4k_site_key_major(const K4ReadSet s, uint32_t m, const uint32_t* __restrict__ idx, uint64_t* __restrict__ key) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  const k4_hit h = s.hit(idx[j]);
  key[j] = ((uint64_t)h.chrom_id << 32) | k4d_adj_start(h);
}

// the 2-bit codes of eight bases (first base in bits 15..14) reversed and complemented
K4_DEV uint32_t k4d_revcomp8(uint32_t x) {
  x = ~x & 0xFFFFu;
  x = ((x & 0x00FFu) << 8) | (x >> 8);
  x = ((x & 0x0F0Fu) << 4) | ((x >> 4) & 0x0F0Fu);
  x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
  return x;
}

// :8757-8808.  key[j] = strand << 16 | octamer, or K4_SITE_UNCOUNTED; site[j] = chrom << 32 | HitLoci
__global__ void __launch_bounds__(256) k4k_site_octamers(K4DevIndex ix, const K4ReadSet s, uint32_t m, const uint32_t* __restrict__ order, int32_t ofs,
                                                         uint32_t* __restrict__ key, uint64_t* __restrict__ site) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  const k4_hit h = s.hit(order[j]);
  const bool minus = h.strand != '+';
  uint32_t hl = h.match_loci;
  if (minus) hl = hl + (uint32_t)h.match_len - 1u - (uint32_t)ofs - 7u;
  else hl += (uint32_t)ofs;
  const uint64_t e0 = ix.ent_start[h.chrom_id - 1];
  const uint32_t clen = (uint32_t)(ix.ent_end[h.chrom_id - 1] - e0 + 1);
  // signed -8..-1: HitLoci + 8 wraps below the length and GetSeq returns nothing; a two-segment read is passed over (:8754)
  const bool undefined = hl >= 0xFFFFFFF8u || (h.ext & (K4_EXT_INDEL | K4_EXT_SPLICE)) != 0;
  if (hl + 8u >= clen) hl = clen - 9u;
  site[j] = ((uint64_t)h.chrom_id << 32) | hl;
  uint32_t k = K4_SITE_UNCOUNTED;
  if (!undefined && clen >= 9u) {  // (a sequence shorter than nine bases has no octamer the clamp could reach)
    const uint64_t pos = e0 + hl;
    const uint32_t* p = ix.ref2 + (pos >> 4);
    const uint32_t sh = (uint32_t)(pos & 15) * 2;
    const uint64_t win = (((uint64_t)p[0] << 32) | p[1]) << sh;  // (the pad behind the last base covers p[1])
    uint32_t oct = (uint32_t)(win >> 48);
    bool clean = true;
    if (k4d_any_exc(ix, (int64_t)pos, (int64_t)pos + 8))  // a flagged block: the exact symbols decide
      for (uint32_t q = 0; q < 8 && clean; q++) clean = k4d_ref_base(ix, pos + q) <= 3u;
    if (clean) k = (minus ? 0x10000u | k4d_revcomp8(oct) : oct);
  }
  key[j] = k;
}

struct IsCounted {
  const uint32_t* key;
  __device__ bool operator()(uint32_t j) const { return key[j] != K4_SITE_UNCOUNTED; }
};

// behind the compaction: v[c] = key << 1 | head (:8812-8819)
__global__ void __launch_bounds__(256) k4k_site_heads(uint32_t n, const uint32_t* __restrict__ cidx, const uint32_t* __restrict__ key,
                                                      const uint64_t* __restrict__ site, uint32_t* __restrict__ v) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n) return;
  const uint32_t j = cidx[c];
  const bool head = c == 0 || site[cidx[c - 1]] != site[j];
  v[c] = (key[j] << 1) | (head ? 1u : 0u);
}

// tab[key] = NumOccs, tab[2 * K4_SITE_OCTS + key] = NumSites.  A stack of reads on one site is a run of equal keys in walk order
// and one hot octamer (poly-A) meets itself in every wave: up to K4_SITE_LEADERS groups of equal keys are added once each.
__global__ void __launch_bounds__(256) k4k_site_hist_atomic(uint32_t n, const uint32_t* __restrict__ v, uint32_t* __restrict__ tab) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  const bool valid = c < n;
  const uint32_t x = valid ? v[c] : 0u;
  const uint32_t k = x >> 1;
  const uint64_t heads = __ballot(valid && (x & 1u));
  uint64_t todo = __ballot(valid);
  const uint32_t lane = threadIdx.x & 63u;
  for (int r = 0; r < K4_SITE_LEADERS && todo; r++) {
    const int lead = __ffsll((unsigned long long)todo) - 1;
    const uint32_t k0 = (uint32_t)__shfl((int)k, lead, 64);
    const uint64_t same = __ballot(valid && k == k0) & todo;
    if (lane == (uint32_t)lead) {
      atomicAdd(&tab[k0], (uint32_t)__popcll(same));
      const uint32_t hs = (uint32_t)__popcll(same & heads);
      if (hs) atomicAdd(&tab[2 * K4_SITE_OCTS + k0], hs);
    }
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) {
    atomicAdd(&tab[k], 1u);
    if (x & 1u) atomicAdd(&tab[2 * K4_SITE_OCTS + k], 1u);
  }
}

// the sort form: run r of the sorted v has value uniq[r] = key << 1 | head and cnt[r] members; a key has at most two runs
__global__ void __launch_bounds__(256) k4k_site_hist_runs(const uint32_t* __restrict__ n_runs, const uint32_t* __restrict__ uniq,
                                                          const uint32_t* __restrict__ cnt, uint32_t* __restrict__ tab) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= *n_runs) return;
  const uint32_t x = uniq[r], k = x >> 1;
  if (k >= 2 * K4_SITE_OCTS) return;
  atomicAdd(&tab[k], cnt[r]);
  if (x & 1u) tab[2 * K4_SITE_OCTS + k] = cnt[r];
}

bool sort_form() {
  const char* e = getenv("K4_SITEPREFS_HIST");
  return e && strcmp(e, "sort") == 0;
}

}  // namespace

extern "C" int k4_site_prefs_dev(k4_index* ix, int pe, int64_t n_reads, int32_t max_ml, int32_t ofs, const void* d_rr, const void* d_hits,
                                 const void* d_pe, k4_site_prefs* out, void* stream) {
  if (!ix || !out) return K4_ERR_PARAMS;
  memset(out, 0, sizeof(*out));
  if (ofs < -100 || ofs > 100) return k4_fail(ix, K4_ERR_PARAMS, "site preferences offset %d outside of range -100..100", (int)ofs);
  if (n_reads < 0) return k4_fail(ix, K4_ERR_PARAMS, "read count out of range");
  K4ReadSet s;
  K4_TRY(k4s_read_set(ix, pe, n_reads, d_rr, d_hits, max_ml, d_pe, nullptr, nullptr, nullptr, nullptr, K4RS_HITS, &s));
  if (n_reads >= 0xFFFFFF00ll) return k4_fail(ix, K4_ERR_PARAMS, "at most 2^32-256 reads per call");
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* blk = (uint32_t*)calloc((size_t)4 * K4_SITE_OCTS, 4);
  if (!blk) return k4_fail(ix, K4_ERR_MEM, "out of memory");
  out->block = blk;
  out->num_occs[0] = blk;
  out->num_occs[1] = blk + K4_SITE_OCTS;
  out->num_sites[0] = blk + 2 * K4_SITE_OCTS;
  out->num_sites[1] = blk + 3 * K4_SITE_OCTS;
  auto run = [&]() -> int {
    if (n_reads == 0) return k4_check_hip(ix, hipStreamSynchronize(st), "stream");
    // 1. the walk order
    K4DevBuf idx0, idx1, mk0, mk1, kk0, kk1;
    uint64_t m64 = 0;
    K4_TRY(k4s_select_indices(ix, idx0, (size_t)n_reads, IsSiteRead{s, ix->d.n_entries}, st, &m64));
    out->n_accepted = m64;
    if (m64 == 0) return K4_OK;
    const uint32_t m = (uint32_t)m64;
    const unsigned mb = (m + 255u) / 256u;
    K4_HIP(ix, idx1.alloc((size_t)m * 4));
    K4_HIP(ix, mk0.alloc((size_t)m * 4));
    K4_HIP(ix, mk1.alloc((size_t)m * 4));
    K4_HIP(ix, kk0.alloc((size_t)m * 8));
    K4_HIP(ix, kk1.alloc((size_t)m * 8));
    hipLaunchKernelGGL(k4k_site_key_minor, dim3(mb), dim3(256), 0, st, s, m, idx0.as<uint32_t>(), mk0.as<uint32_t>());
    K4_HIP(ix, hipGetLastError());
    rocprim::double_buffer<uint32_t> mk(mk0.as<uint32_t>(), mk1.as<uint32_t>());
    rocprim::double_buffer<uint32_t> vb(idx0.as<uint32_t>(), idx1.as<uint32_t>());
    K4_TRY(k4s_sort_pairs<K4DevBuf>(ix, mk, vb, (size_t)m, 0u, 32u, st));
    hipLaunchKernelGGL(k4k_site_key_major, dim3(mb), dim3(256), 0, st, s, m, vb.current(), kk0.as<uint64_t>());
    K4_HIP(ix, hipGetLastError());
    rocprim::double_buffer<uint64_t> kk(kk0.as<uint64_t>(), kk1.as<uint64_t>());
    unsigned top = 33;  // key = chrom << 32 | start: only the bits chromosome ids can reach are sorted on
    while (top < 64 && (ix->d.n_entries >> (top - 32)) != 0) top++;
    K4_TRY(k4s_sort_pairs<K4DevBuf>(ix, kk, vb, (size_t)m, 0u, top, st));
    // 2. octamer and locus per sorted read (the sort's buffers are done with: the keys and loci go where they were)
    uint32_t* key = mk0.as<uint32_t>();
    uint64_t* site = kk.alternate();
    hipLaunchKernelGGL(k4k_site_octamers, dim3(mb), dim3(256), 0, st, ix->d, s, m, vb.current(), ofs, key, site);
    K4_HIP(ix, hipGetLastError());
    // 3. the counted reads, in walk order, and their site heads
    K4DevBuf cidx, tab;
    uint64_t n64 = 0;
    K4_TRY(k4s_select_indices(ix, cidx, (size_t)m, IsCounted{key}, st, &n64));
    out->n_counted = n64;
    if (n64 == 0) return K4_OK;
    const uint32_t n = (uint32_t)n64;
    const unsigned nb = (n + 255u) / 256u;
    uint32_t* v = mk1.as<uint32_t>();
    hipLaunchKernelGGL(k4k_site_heads, dim3(nb), dim3(256), 0, st, n, cidx.as<uint32_t>(), key, site, v);
    K4_HIP(ix, hipGetLastError());
    // 4. the tables
    K4_HIP(ix, tab.alloc((size_t)4 * K4_SITE_OCTS * 4));
    K4_HIP(ix, hipMemsetAsync(tab.p, 0, (size_t)4 * K4_SITE_OCTS * 4, st));
    if (sort_form()) {
      K4DevBuf uq, rc, nr;
      K4_HIP(ix, uq.alloc((size_t)4 * K4_SITE_OCTS * 4));  // (at most 2^18 distinct values)
      K4_HIP(ix, rc.alloc((size_t)4 * K4_SITE_OCTS * 4));
      K4_HIP(ix, nr.alloc(8));
      rocprim::double_buffer<uint32_t> sv(v, idx0.as<uint32_t>() == vb.current() ? idx1.as<uint32_t>() : idx0.as<uint32_t>());
      K4_TRY(k4s_sort_keys<K4DevBuf>(ix, sv, (size_t)n, 0u, 18u, st));
      const uint32_t* sorted = sv.current();
      K4_TRY(k4s_two_calls<K4DevBuf>(ix, "rocprim::run_length_encode", [&](void* t, size_t& tb) {
        return rocprim::run_length_encode(t, tb, sorted, (unsigned)n, uq.as<uint32_t>(), rc.as<uint32_t>(), nr.as<uint32_t>(), st);
      }));
      hipLaunchKernelGGL(k4k_site_hist_runs, dim3(4 * K4_SITE_OCTS / 256), dim3(256), 0, st, nr.as<uint32_t>(), uq.as<uint32_t>(), rc.as<uint32_t>(),
                         tab.as<uint32_t>());
    } else
      hipLaunchKernelGGL(k4k_site_hist_atomic, dim3(nb), dim3(256), 0, st, n, v, tab.as<uint32_t>());
    K4_HIP(ix, hipGetLastError());
    K4_HIP(ix, hipMemcpyAsync(blk, tab.p, (size_t)4 * K4_SITE_OCTS * 4, hipMemcpyDeviceToHost, st));
    return k4_check_hip(ix, hipStreamSynchronize(st), "k4_site_prefs_dev");
  };
  const int rc = run();
  if (rc != K4_OK) k4_free_site_prefs(out);
  return rc;
}

extern "C" void k4_free_site_prefs(k4_site_prefs* s) {
  if (!s) return;
  free(s->block);
  memset(s, 0, sizeof(*s));
}

// The scale step (:8823-8872) and the text (:8910-8945).  The reference sorts the 65536 entries of a strand ascending by
// NumOccs / NumSites with an unstable quicksort; here the sort is stable, i.e. ties are broken by octamer ascending, and the top
// 64 are summed in ascending order of value.  The counters are `int` there and are printed with %d.
extern "C" int k4_write_site_prefs(const k4_site_prefs* s, const char* path) {
  if (!s || !path || !path[0]) return K4_ERR_PARAMS;
  std::string o;
  if (s->block && s->n_accepted > 0) {  // (:743, :780: only when a read was accepted; the file stays empty otherwise)
    o.reserve((size_t)5 << 20);
    o += "\"Id\",\"Strand\",\"Octamer\",\"TotalHits\",\"UniqueLoci\",\"RelScale\"\n";
    std::vector<double> rel(K4_SITE_OCTS);
    std::vector<uint32_t> by(K4_SITE_OCTS);
    for (int strand = 0; strand < 2; strand++) {
      const uint32_t *occ = s->num_occs[strand], *sites = s->num_sites[strand];
      for (uint32_t k = 0; k < K4_SITE_OCTS; k++) {
        rel[k] = sites[k] >= 1 ? (double)(int)occ[k] / (int)sites[k] : 0.0;
        by[k] = k;
      }
      std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return rel[a] < rel[b]; });
      double top = 0.0;
      for (uint32_t q = 0xffc0; q < K4_SITE_OCTS; q++) { top += rel[by[q]]; rel[by[q]] = 1.0; }
      top /= 64;
      for (uint32_t q = 0; q < 0xffc0; q++)
        if (rel[by[q]] > 0.0) rel[by[q]] = std::max(0.0001, rel[by[q]] / top);
      char line[96];
      for (uint32_t k = 0; k < 0xffff; k++) {  // (the reference's loop ends one short: tttttttt is never written)
        char oct[9];
        for (int q = 0; q < 8; q++) oct[q] = "acgt"[(k >> (14 - 2 * q)) & 3u];
        oct[8] = 0;
        const int len = snprintf(line, sizeof(line), "%d,\"%c\",\"%s\",%d,%d,%1.3f\n", (int)(k + 1), strand ? '-' : '+', oct, (int)occ[k],
                                 (int)sites[k], rel[k]);
        o.append(line, (size_t)len);
      }
    }
  }
  FILE* fp = fopen(path, "wb");
  bool ok = fp && fwrite(o.data(), 1, o.size(), fp) == o.size();
  if (fp && fclose(fp) != 0) ok = false;
  if (!ok) {
    k4_set_global_error("unable to write %s", path);
    return K4_ERR_CREATE_FILE;
  }
  return K4_OK;
}
