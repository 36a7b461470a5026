// kit4b_amd/csrc/k4_stats.hip -- `kalign -O <file>`: the alignment statistics files, counted on the device over the records the
// align entry points and the global stages left in HBM, printed on the host:
//   k4_align_stats_dev    <- CKAligner::WriteSubDist          ngskit4b/KAligner.cpp:6469-6525 (substitutions by read position and
//                                                              quality band, mismatches per read, m_MaxAlignLen)
//                            CKAligner::ReportTargHitCnts      :5458-5712 (per target: alignments, distinct start loci, leading trimers)
//                            m_MultiHitDist (:9943) and m_pLenDist (:3251, :3408, :3511), tallied while the reads are aligned
//   k4_write_align_stats  <- CKAligner::WriteBasicCountStats  :4159-4300, ReportTargHitCnts' text, ProcessPairedEnds :3092-3146
//
// Every figure is a count over a set of reads, so nothing here depends on the order the reads are walked in.
//   k4k_sub_dist     one wave per read, a lane per read position: the read bytes of a wave load are consecutive, sixteen lanes
//                    share a packed reference word, and the 64 LDS atomics of one wave instruction go to 64 different
//                    positions -- and for an untrimmed read to the same position every time, so its first 128 positions are
//                    counted in the lane's registers.  A block keeps 4 bands x Lt positions x {instances, substitutions} as 32-bit counters in LDS
//                    (Lt = the call's longest read, at most K4_STATS_LDS_LEN), positions behind Lt go to the global 64-bit
//                    table directly; the block's non-zero counters are added to the global table once, at its end.
//   k4k_targ_counts  one thread per read: the (chrom, start) key of the distinct-loci sort, and indeterminate / trimer counts
//                    per target in an LDS table while n_entries x 65 counters fit K4_STATS_LDS_ENT, else by global atomics
//                    (with 10^5 targets the reads of a wave rarely meet on one counter).
//   k4k_uniq_heads   over the sorted keys: run heads per target; a block whose keys share one target adds once.
//   k4k_multi_tally  LowHitInstances of the reads AlignRead accepted, as the align step left it (the later stages zero it).
#include <hip/hip_runtime.h>
#include <stdarg.h>
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

#define K4_STATS_LDS_LEN 1024   // read positions of the block's LDS table (32 KB of counters: four blocks per CU)
#define K4_STATS_LDS_MSUB 256   // mismatches-per-read bins kept in LDS
#define K4_STATS_LDS_ENT 8192   // per-target counters (n_entries x 65) kept in LDS: up to 126 targets
#define K4_STATS_ENT_W 65       // per target: [0] reads whose leading trimer holds a non-ACGT, [1 + t] reads that start with trimer t

namespace {

// WriteSubDist (:6469-6525).  The read is walked in read orientation from ReadOfs + TrimLeft (Seg[0].ReadOfs is 0) to
// ReadLen - TrimRight; the target window is AdjHitLen bases from AdjStartLoci, reverse complemented for a '-' hit, and is walked
// from its first element.
__global__ void __launch_bounds__(256) k4k_sub_dist(K4DevIndex ix, const K4ReadSet s, uint32_t Lt, uint32_t L,
                                                    unsigned long long* __restrict__ g_insts,
                                                    unsigned long long* __restrict__ g_subs, unsigned long long* __restrict__ g_msub,
                                                    uint32_t* __restrict__ g_maxlen) {
  extern __shared__ uint32_t lds[];
  uint32_t* tab = lds;                           // [(band * Lt + pos) * 2 + {0: QInsts, 1: Subs}]
  uint32_t* msub = lds + 8 * Lt;                 // [K4_STATS_LDS_MSUB]
  uint32_t* smax = msub + K4_STATS_LDS_MSUB;     // [1]
  for (uint32_t k = threadIdx.x; k < 8 * Lt + K4_STATS_LDS_MSUB + 1; k += 256) lds[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t wmax = 0;
  // An untrimmed read puts positions lane and 64 + lane on this lane every time: those are counted in registers (per band, no
  // atomic at all) and added to the LDS table once, behind the loop.  Trimmed reads and positions from 128 on go to LDS directly.
  uint32_t ri[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, rsub[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < s.n_reads; i += (int64_t)gridDim.x * 4) {
    k4_hit h;
    if (!s.accepted(i, h)) continue;
    if (h.ext & (K4_EXT_INDEL | K4_EXT_SPLICE)) continue;  // FlagSegs: a two-segment read is sloughed (:6480)
    if (h.chrom_id == 0 || h.chrom_id > ix.n_entries) continue;
    const uint32_t len = s.lens[i];
    const uint32_t tl = K4_HIT_TRIM_LEFT(h), tr = K4_HIT_TRIM_RIGHT(h);
    wmax = max(wmax, len);
    const bool minus = h.strand == '-';
    const uint32_t adj_start = k4d_adj_start(h);
    const int32_t adj_len = (int32_t)k4d_adj_len(h);
    const uint32_t start = tl;
    // (a one-segment hit spans the whole read, so the walk is AdjHitLen long; the bounds keep an odd record inside the tables)
    uint32_t end = len > tr ? len - tr : 0u;
    if (adj_len <= 0) end = 0;
    else if (end > start + (uint32_t)adj_len) end = start + (uint32_t)adj_len;
    if (end > L) end = L;
    const uint8_t* rd = s.reads + s.offs[i];
    const uint64_t base = ix.ent_start[h.chrom_id - 1] + adj_start;
    // position p of the read: its quality band, and whether it differs from the target
    auto look = [&](uint32_t p, uint32_t& band) -> bool {
      const uint32_t b = rd[p];
      band = (b >> 6) & 3u;  // the 4-bit score 0..3 | 4..7 | 8..11 | 12..15
      const uint32_t j = p - start;
      const uint64_t pos = base + (minus ? (uint32_t)adj_len - 1u - j : j);
      uint32_t t = pos < ix.n ? k4d_ref_base(ix, pos) : 7u;
      if (minus && t <= 3u) t = 3u - t;  // CSeqTrans::ReverseComplement leaves the other symbols as they are
      return (b & 7u) != (t & 7u);
    };
    uint32_t nm = 0, p_from = start + (uint32_t)lane;
    if (start == 0) {
#pragma unroll
      for (int c = 0; c < 2; c++) {
        const uint32_t p = 64u * c + (uint32_t)lane;
        if (p < end) {
          uint32_t band;
          const bool mm = look(p, band);
#pragma unroll
          for (uint32_t q = 0; q < 4; q++) {
            ri[c][q] += band == q ? 1u : 0u;
            rsub[c][q] += (band == q && mm) ? 1u : 0u;
          }
          nm += mm ? 1u : 0u;
        }
      }
      p_from = 128u + (uint32_t)lane;
    }
    for (uint32_t p = p_from; p < end; p += 64u) {
      uint32_t band;
      const bool mm = look(p, band);
      if (p < Lt) {
        uint32_t* c = tab + ((size_t)band * Lt + p) * 2;
        atomicAdd(c, 1u);
        if (mm) atomicAdd(c + 1, 1u);
      } else {
        atomicAdd(&g_insts[(size_t)band * L + p], 1ull);
        if (mm) atomicAdd(&g_subs[(size_t)band * L + p], 1ull);
      }
      nm += mm ? 1u : 0u;
    }
    for (int d = 32; d > 0; d >>= 1) nm += __shfl_xor(nm, d, 64);
    if (lane == 0) {
      if (nm < K4_STATS_LDS_MSUB) atomicAdd(&msub[nm], 1u);
      else atomicAdd(&g_msub[min(nm, L)], 1ull);
    }
  }
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const uint32_t p = 64u * c + (uint32_t)lane;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      if (ri[c][q] && p < Lt) atomicAdd(tab + ((size_t)q * Lt + p) * 2, ri[c][q]);  // (p < end <= L <= Lt whenever it was counted)
      if (rsub[c][q] && p < Lt) atomicAdd(tab + ((size_t)q * Lt + p) * 2 + 1, rsub[c][q]);
    }
  }
  if (lane == 0 && wmax) atomicMax(smax, wmax);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < 8 * Lt; k += 256) {
    const uint32_t v = tab[k];
    if (!v) continue;
    const uint32_t cell = k >> 1, band = cell / Lt, p = cell - band * Lt;
    if (p >= L) continue;
    atomicAdd(((k & 1u) ? g_subs : g_insts) + (size_t)band * L + p, (unsigned long long)v);
  }
  for (uint32_t k = threadIdx.x; k < K4_STATS_LDS_MSUB; k += 256)
    if (msub[k]) atomicAdd(&g_msub[min(k, L)], (unsigned long long)msub[k]);
  if (threadIdx.x == 0 && *smax) atomicMax(g_maxlen, *smax);
}

// ReportTargHitCnts (:5586-5612): per accepted read the leading trimer of the read as loaded, and AdjAlignStartLoci
__global__ void __launch_bounds__(256) k4k_targ_counts(uint32_t n_entries, const K4ReadSet s, int use_lds, uint64_t* __restrict__ keys, uint32_t* __restrict__ g_ent,
                                                       unsigned long long* __restrict__ g_nacc) {
  extern __shared__ uint32_t lds[];
  const uint32_t n_cnt = use_lds ? n_entries * K4_STATS_ENT_W : 0u;
  for (uint32_t k = threadIdx.x; k < n_cnt; k += 256) lds[k] = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.n_reads; i += (int64_t)gridDim.x * 256) {
    k4_hit h;
    const bool acc = s.accepted(i, h) && h.chrom_id >= 1 && h.chrom_id <= n_entries;
    if (!acc) { keys[i] = ~0ull; continue; }
    keys[i] = ((uint64_t)h.chrom_id << 32) | k4d_adj_start(h);
    mine++;
    uint32_t slot = 0, tri = 0;
    if (s.lens[i] >= 3) {  // (no read is that short behind the length filter; one that were counts as indeterminate)
      const uint8_t* rd = s.reads + s.offs[i];
      bool indet = false;
      for (int q = 0; q < 3 && !indet; q++) {
        const uint32_t b = rd[q] & 7u;
        if (b > 3u) indet = true;
        else tri = (tri << 2) | b;
      }
      if (!indet) slot = 1 + tri;
    }
    const uint32_t at = (h.chrom_id - 1) * K4_STATS_ENT_W + slot;
    if (use_lds) atomicAdd(&lds[at], 1u);
    else atomicAdd(&g_ent[at], 1u);
  }
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(g_nacc, (unsigned long long)mine);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < n_cnt; k += 256)
    if (lds[k]) atomicAdd(&g_ent[k], lds[k]);
}

// distinct AdjAlignStartLoci per target: the heads of the runs of equal keys
__global__ void __launch_bounds__(256) k4k_uniq_heads(uint64_t m, const uint64_t* __restrict__ keys, uint32_t n_entries,
                                                      uint32_t* __restrict__ uniq) {
  const uint64_t j0 = (uint64_t)blockIdx.x * 256, j = j0 + threadIdx.x;
  const uint64_t last = min(j0 + 255, m - 1);
  const uint32_t c_first = (uint32_t)(keys[j0] >> 32), c_last = (uint32_t)(keys[last] >> 32);
  bool head = false;
  uint32_t chrom = 0;
  if (j < m) {
    const uint64_t k = keys[j];
    chrom = (uint32_t)(k >> 32);
    head = k != ~0ull && (j == 0 || keys[j - 1] != k) && chrom >= 1 && chrom <= n_entries;
  }
  if (c_first == c_last) {  // sorted: the whole block lies on one target
    const int c = __syncthreads_count(head);
    if (threadIdx.x == 0 && c) atomicAdd(&uniq[c_first - 1], (uint32_t)c);
  } else if (head)
    atomicAdd(&uniq[chrom - 1], 1u);
}

// m_MultiHitDist[LowHitInstances - 1] += 1 for a read AlignRead took as eHRhits outside of eMLall (:9902-9943)
__global__ void __launch_bounds__(256) k4k_multi_tally(int64_t n, const k4_read_result* __restrict__ rr,
                                                       unsigned long long* __restrict__ multi) {
  __shared__ uint32_t hist[K4_STATS_MULTI];
  for (uint32_t k = threadIdx.x; k < K4_STATS_MULTI; k += 256) hist[k] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const k4_read_result r = rr[i];
    if (r.hit_rslt == K4_HR_HITS && r.inst > 0) atomicAdd(&hist[min(r.inst, K4_STATS_MULTI) - 1], 1u);
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < K4_STATS_MULTI; k += 256)
    if (hist[k]) atomicAdd(&multi[k], (unsigned long long)hist[k]);
}

unsigned grid_for(int64_t items_per_block_units, int64_t n) {
  const int64_t want = (n + items_per_block_units - 1) / items_per_block_units;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, 256 * 8));
}

}  // namespace

// the run tallies: [0, K4_STATS_MULTI) multihit distribution, then K4_STATS_PE_LEN + 1 insert lengths
#define K4_RUN_STATS_WORDS ((size_t)K4_STATS_MULTI + K4_STATS_PE_LEN + 1)

extern "C" int k4_align_stats_collect(k4_index* ix, int on) {
  if (!ix) return K4_ERR_PARAMS;
  K4_HIP(ix, hipSetDevice(ix->device));
  if (!on) {
    ix->d_run_stats.release();
    return K4_OK;
  }
  K4_HIP(ix, ix->d_run_stats.reserve(K4_RUN_STATS_WORDS * 8));
  K4_HIP(ix, hipMemset(ix->d_run_stats.p, 0, K4_RUN_STATS_WORDS * 8));
  return K4_OK;
}

// k4_align.hip calls this behind the classification of a batch (k4_kalign_*_batch_dev; the SE pass of a PE batch as well)
int k4i_stats_tally_multi(k4_index* ix, const void* d_rr, int64_t n, void* stream) {
  if (!ix->d_run_stats.p || n <= 0) return K4_OK;
  hipLaunchKernelGGL(k4k_multi_tally, dim3(grid_for(256 * 16, n)), dim3(256), 0, (hipStream_t)stream, n, (const k4_read_result*)d_rr,
                     ix->d_run_stats.as<unsigned long long>());
  return k4_check_hip(ix, hipGetLastError(), "k4k_multi_tally");
}
unsigned long long* k4i_stats_pe_len_dist(k4_index* ix) { return ix->d_run_stats.p ? ix->d_run_stats.as<unsigned long long>() + K4_STATS_MULTI : nullptr; }

extern "C" int k4_align_stats_dev(k4_index* ix, int pe, int64_t n_reads, int32_t max_ml, int32_t max_read_len, const void* d_rr,
                                  const void* d_hits, const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens,
                                  k4_align_stats* out, void* stream) {
  if (!ix || !out) return K4_ERR_PARAMS;
  memset(out, 0, sizeof(*out));
  if (n_reads < 0 || max_read_len < 0 || max_read_len > K4_MAX_READ_LEN) return k4_fail(ix, K4_ERR_PARAMS, "read count / length out of range");
  K4ReadSet src;
  K4_TRY(k4s_read_set(ix, pe, n_reads, d_rr, d_hits, max_ml, d_pe, nullptr, d_reads, d_offs, d_lens, K4RS_HITS | K4RS_READS, &src));
  if (n_reads >= 0xFFFFFF00ll) return k4_fail(ix, K4_ERR_PARAMS, "at most 2^32-256 reads per call");
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  const uint32_t L = (uint32_t)std::max<int32_t>(max_read_len, 1), ne = ix->d.n_entries;
  // host block: q_insts[4][L] q_subs[4][L] m_sub[L+1] multi_hit[] pe_len_dist[] (u64), then the per-target u32 arrays
  const size_t n64 = (size_t)8 * L + (L + 1) + K4_RUN_STATS_WORDS;
  const size_t n32 = (size_t)ne * (3 + 64);
  uint8_t* blk = (uint8_t*)calloc(n64 * 8 + n32 * 4 + 8, 1);
  if (!blk) return k4_fail(ix, K4_ERR_MEM, "out of memory");
  out->block = blk;
  out->len_stride = L;
  out->n_entries = ne;
  out->q_insts = (uint64_t*)blk;
  out->q_subs = out->q_insts + (size_t)4 * L;
  out->m_sub = out->q_subs + (size_t)4 * L;
  out->multi_hit = out->m_sub + (L + 1);
  out->pe_len_dist = out->multi_hit + K4_STATS_MULTI;
  out->ent_hits = (uint32_t*)(blk + n64 * 8);
  out->ent_uniq_loci = out->ent_hits + ne;
  out->ent_indeterminate = out->ent_uniq_loci + ne;
  out->ent_trimer = out->ent_indeterminate + ne;
  auto fail = [&](int rc) { free(blk); memset(out, 0, sizeof(*out)); return rc; };
  int rc;
  if (ix->d_run_stats.p) {
    if ((rc = k4_check_hip(ix, hipStreamSynchronize(st), "stream")) != K4_OK) return fail(rc);
    if ((rc = k4_check_hip(ix, hipMemcpy(out->multi_hit, ix->d_run_stats.p, K4_RUN_STATS_WORDS * 8, hipMemcpyDeviceToHost), "run tallies")) != K4_OK)
      return fail(rc);
  }
  if (n_reads == 0) return K4_OK;
  // device block: the position tables and m_sub (u64), accepted count (u64), max length, the per-target table and the distinct loci (u32)
  const size_t d64 = (size_t)8 * L + (L + 1) + 1;
  const size_t d32 = 2 + (size_t)ne * (K4_STATS_ENT_W + 1);
  K4DevBuf dev, k0, k1;
  if ((rc = k4_check_hip(ix, dev.alloc(d64 * 8 + d32 * 4), "hipMalloc(stats)")) != K4_OK) return fail(rc);
  if ((rc = k4_check_hip(ix, hipMemsetAsync(dev.p, 0, d64 * 8 + d32 * 4, st), "hipMemset(stats)")) != K4_OK) return fail(rc);
  unsigned long long* g_insts = dev.as<unsigned long long>();
  unsigned long long* g_subs = g_insts + (size_t)4 * L;
  unsigned long long* g_msub = g_subs + (size_t)4 * L;
  unsigned long long* g_nacc = g_msub + (L + 1);
  uint32_t* g_maxlen = (uint32_t*)(g_nacc + 1);
  uint32_t* g_ent = g_maxlen + 2;
  uint32_t* g_uniq = g_ent + (size_t)ne * K4_STATS_ENT_W;
  const uint32_t Lt = std::min<uint32_t>((L + 63u) & ~63u, K4_STATS_LDS_LEN);
  hipLaunchKernelGGL(k4k_sub_dist, dim3(grid_for(4 * 64, n_reads)), dim3(256), (8 * Lt + K4_STATS_LDS_MSUB + 1) * 4, st, ix->d, src, Lt, L,
                     g_insts, g_subs, g_msub, g_maxlen);
  if ((rc = k4_check_hip(ix, hipGetLastError(), "k4k_sub_dist")) != K4_OK) return fail(rc);
  if ((rc = k4_check_hip(ix, k0.alloc((size_t)n_reads * 8), "hipMalloc(stats keys)")) != K4_OK) return fail(rc);
  if ((rc = k4_check_hip(ix, k1.alloc((size_t)n_reads * 8), "hipMalloc(stats keys)")) != K4_OK) return fail(rc);
  const int use_lds = (size_t)ne * K4_STATS_ENT_W <= K4_STATS_LDS_ENT ? 1 : 0;
  hipLaunchKernelGGL(k4k_targ_counts, dim3(grid_for(256 * 16, n_reads)), dim3(256), use_lds ? (size_t)ne * K4_STATS_ENT_W * 4 : 0, st, ne, src,
                     use_lds, k0.as<uint64_t>(), g_ent, g_nacc);
  if ((rc = k4_check_hip(ix, hipGetLastError(), "k4k_targ_counts")) != K4_OK) return fail(rc);
  rocprim::double_buffer<uint64_t> kk(k0.as<uint64_t>(), k1.as<uint64_t>());
  if ((rc = k4s_sort_keys<K4DevBuf>(ix, kk, (size_t)n_reads, 0u, 64u, st)) != K4_OK) return fail(rc);
  hipLaunchKernelGGL(k4k_uniq_heads, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, st, (uint64_t)n_reads, kk.current(), ne, g_uniq);
  if ((rc = k4_check_hip(ix, hipGetLastError(), "k4k_uniq_heads")) != K4_OK) return fail(rc);
  // down: the u64 tables are laid out as in the host block; the per-target table is unpacked
  std::vector<uint32_t> ent(d32);
  uint64_t nacc = 0;
  if ((rc = k4_check_hip(ix, hipMemcpyAsync(out->q_insts, g_insts, ((size_t)8 * L + (L + 1)) * 8, hipMemcpyDeviceToHost, st), "copy")) != K4_OK) return fail(rc);
  if ((rc = k4_check_hip(ix, hipMemcpyAsync(&nacc, g_nacc, 8, hipMemcpyDeviceToHost, st), "copy")) != K4_OK) return fail(rc);
  if ((rc = k4_check_hip(ix, hipMemcpyAsync(ent.data(), g_maxlen, d32 * 4, hipMemcpyDeviceToHost, st), "copy")) != K4_OK) return fail(rc);
  if ((rc = k4_check_hip(ix, hipStreamSynchronize(st), "k4_align_stats_dev")) != K4_OK) return fail(rc);
  out->n_accepted = nacc;
  out->max_align_len = ent[0];
  for (uint32_t e = 0; e < ne; e++) {
    const uint32_t* row = ent.data() + 2 + (size_t)e * K4_STATS_ENT_W;
    uint32_t hits = row[0];
    for (int t = 0; t < 64; t++) { out->ent_trimer[(size_t)e * 64 + t] = row[1 + t]; hits += row[1 + t]; }
    out->ent_hits[e] = hits;
    out->ent_indeterminate[e] = row[0];
    out->ent_uniq_loci[e] = ent[2 + (size_t)ne * K4_STATS_ENT_W + e];
  }
  return K4_OK;
}

extern "C" void k4_free_align_stats(k4_align_stats* s) {
  if (!s) return;
  free(s->block);
  memset(s, 0, sizeof(*s));
}

// ---- the three files ------------------------------------------------------------------------------------------------------
namespace {
void put(std::string& o, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void put(std::string& o, const char* fmt, ...) {
  char b[256];
  va_list ap;
  va_start(ap, fmt);
  const int k = vsnprintf(b, sizeof(b), fmt, ap);
  va_end(ap);
  if (k > 0) o.append(b, (size_t)std::min<int>(k, (int)sizeof(b) - 1));
}
bool write_file(const std::string& path, const std::string& text) {
  FILE* fp = fopen(path.c_str(), "wb");
  if (!fp) return false;
  bool ok = fwrite(text.data(), 1, text.size(), fp) == text.size();
  if (fclose(fp) != 0) ok = false;
  return ok;
}
// CUtility::AppendFileNameSuffix(.., '.'): the name cut at its last '.', unless a path separator comes first
std::string side_name(const std::string& path, const char* suffix) {
  std::string stem = path;
  for (size_t q = stem.size(); q > 0; q--) {
    if (stem[q - 1] == '.') { stem.resize(q - 1); break; }
    if (stem[q - 1] == '/' || stem[q - 1] == '\\') break;
  }
  return stem + suffix;
}
}  // namespace

// The reference keeps these counters as `int` and prints them with %d: a count past 2^31-1 prints as the wrapped value there, and here.
extern "C" int k4_write_align_stats(k4_index* ix, const k4_align_stats* s, uint64_t n_loaded, int32_t ml_mode, int32_t max_multi, int pe,
                                    const char* path) {
  if (!ix || !s || !path || !path[0]) return K4_ERR_PARAMS;
  if (!s->block) return k4_fail(ix, K4_ERR_PARAMS, "k4_write_align_stats: the statistics were not filled (k4_align_stats_dev)");
  if (max_multi < 0 || max_multi > K4_STATS_MULTI) return k4_fail(ix, K4_ERR_PARAMS, "max_multi outside of 0..%d", K4_STATS_MULTI);
  const std::string base = path;
  if (pe) {  // ProcessPairedEnds :3092-3146, whatever was accepted
    std::string o;
    for (int k = 0; k <= K4_STATS_PE_LEN; k++) put(o, "%d,%d\n", k, (int)s->pe_len_dist[k]);
    const std::string fn = side_name(base, ".GlobalPEInsertDist.csv");
    if (!write_file(fn, o)) return k4_fail(ix, K4_ERR_CREATE_FILE, "unable to write %s", fn.c_str());
  }
  const bool report = s->n_accepted > 0 && s->max_align_len > 0;  // KAligner.cpp:774-778
  std::string o;
  const uint32_t M = std::min(s->max_align_len, s->len_stride), L = s->len_stride;
  if (report) {  // WriteBasicCountStats :4159-4300
    if (ml_mode > 0) {
      o += "\"Multihit distribution\"\n,";
      for (int k = 0; k < max_multi; k++) put(o, ",%d", k + 1);
      o += "\n,,\"Instances\"";
      for (int k = 0; k < max_multi; k++) put(o, ",%d", (int)s->multi_hit[k]);
      o += "\n";
    }
    static const char* const inst_band[4] = {"\n,\"Phred 0..9\"", "\n,\"Phred 10..19\"", "\n,\"Phred 20..29\"", "\n,\"Phred 30+\""};
    static const char* const subs_band[4] = {"\n,\"Phred 0..8\"", "\n,\"Phred 9..19\"", "\n,\"Phred 20..29\"", "\n,\"Phred 30+\""};
    o += "\"Phred Score Instances\"\n,\"Psn\"";
    for (uint32_t p = 0; p < M; p++) put(o, ",%d", (int)(p + 1));
    for (int b = 0; b < 4; b++) {
      o += inst_band[b];
      for (uint32_t p = 0; p < M; p++) put(o, ",%d", (int)s->q_insts[(size_t)b * L + p]);
    }
    o += "\n\"Aligner Induced Subs\"\n,\"Psn\"";
    for (uint32_t p = 0; p < M; p++) put(o, ",%d", (int)(p + 1));
    for (int b = 0; b < 4; b++) {
      o += subs_band[b];
      for (uint32_t p = 0; p < M; p++) put(o, ",%d", (int)s->q_subs[(size_t)b * L + p]);
    }
    o += "\n\"Multiple substitutions\"\n,\"NumSubs\"";
    for (uint32_t p = 0; p < M; p++) put(o, ",%d", (int)p);
    o += "\n,\"Instances\"";
    for (uint32_t p = 0; p < M; p++) put(o, ",%d", (int)s->m_sub[p]);
    o += "\n";
  }
  if (!write_file(base, o)) return k4_fail(ix, K4_ERR_CREATE_FILE, "unable to write %s", base.c_str());
  if (!report) return K4_OK;
  // ReportTargHitCnts :5458-5712
  o.clear();
  o += "\"FeatID\",\"TargSeq\",\"TargLen\",\"NumHits\",\"RPKM\",\"NumUniqueLoci\"";
  for (int t = 0; t < 64; t++) {
    char tri[4] = {"ACGT"[(t >> 4) & 3], "ACGT"[(t >> 2) & 3], "ACGT"[t & 3], 0};
    put(o, ",\"%s\"", tri);
  }
  o += ",Indeterminates\n";
  uint32_t last_hit = 0;  // 1-based id of the last target with alignments
  for (uint32_t e = 0; e < s->n_entries && e < ix->entries.size(); e++)
    if (s->ent_hits[e]) last_hit = e + 1;
  for (uint32_t e = 0; e < s->n_entries && e < ix->entries.size(); e++) {
    const k4_entry& en = ix->entries[e];
    const uint32_t nh = s->ent_hits[e];
    if (!nh) {  // the two zero forms: in front of a target with alignments, and behind the last one
      put(o, "%u,\"%s\",%u,0,0.0,0", e + 1, en.name, en.seq_len);
      for (int t = 0; t < 64; t++) o += (e + 1 < last_hit) ? ",0.0" : ",0";
      o += ",0\n";
      continue;
    }
    double rpkm = ((double)nh * 1000.0f);
    rpkm /= (double)en.seq_len;
    rpkm *= 1000000.0f / (double)n_loaded;
    put(o, "%u,\"%s\",%u,%u,%f,%u", e + 1, en.name, en.seq_len, nh, rpkm, s->ent_uniq_loci[e]);
    for (int t = 0; t < 64; t++) put(o, ",%1.4f", (double)s->ent_trimer[(size_t)e * 64 + t] / (double)nh);
    put(o, ",%u\n", s->ent_indeterminate[e]);
  }
  const std::string fn = side_name(base, ".AlignCntsDist.csv");
  if (!write_file(fn, o)) return k4_fail(ix, K4_ERR_CREATE_FILE, "unable to write %s", fn.c_str());
  return K4_OK;
}
