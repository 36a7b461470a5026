// kit4b_amd/csrc/k4_primer.hip -- `kalign -6 <n>` (`--pcrprimersubs`): 5' PCR random-primer artefact correction on the device, over
// the records the align calls (and the stages behind them) left in HBM and over the reads themselves:
//   k4_pcr5_primer_correct_dev <- CKAligner::PCR5PrimerCorrect  ngskit4b/KAligner.cpp:2115-2226 (called from Align, :642-651)
//
// kalign aligns with MaxSubs + n substitutions per 100 bp (m_InitalAlignSubs, :245-248) and then looks at every accepted one-segment
// read whose Seg[0] spans the whole read: MaxMMs = (MaxSubs * ReadLen + 50) / 100; a read with more mismatches than that has the
// mismatching bases among its first KLen (12) rewritten to the target's base, in read order, until it is within MaxMMs; a read that
// the KLen bases cannot bring there becomes eNARNoHit with NumHits = 0 and stays as it was read (LowHitInstances is not cleared).
// The comparison is on the symbol codes: an N in the read always counts and is rewritten, an N in the target is written into the read.
//
// A lane per read (the work is at most 12 symbols):
//   phase 1  the read's record only: accepted? one segment? Seg[0].MatchLen == ReadLen? LowMMCnt > MaxMMs?  Nearly every lane
//            leaves here.
//   phase 2  the 12 target symbols that face the read's first 12 bases -- 24 bits out of two packed words where the exception bitmap
//            shows no flagged block under the span, the exact reader (K4Tb) otherwise; complemented and taken from the window's end
//            for a Crick alignment -- against the read's first bytes; the reference's two walks; byte stores for the bases that
//            change (reads do not overlap: nothing to synchronise); the record.
// The three totals are summed per wave, then per block in LDS: three atomics per block at the most.
// DESIGN.md "5' PCR primer correction" has the figures.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "k4_device.h"
#include "k4_stage.h"

#define K4_PRIMER_KLEN 12  /* the KLen default of PCR5PrimerCorrect (KAligner.h:850); what kalign always passes */

namespace {

__global__ void __launch_bounds__(256) k4k_primer_correct(K4DevIndex ix, int max_subs, int klen, K4ReadSet rs,
                                                          unsigned long long* __restrict__ totals) {
  __shared__ uint32_t s_tot[3];
  if (threadIdx.x < 3) s_tot[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  // ---- phase 1: the record
  bool todo = false;
  k4_hit h = {0, 0, 0, 0, 0, 0};
  int low_mm = 0, max_mms = 0;
  uint32_t rlen = 0;
  if (i < rs.n_reads && rs.accepted(i, h)) {
    rlen = rs.lens[i];
    low_mm = rs.low_mm(i);
    max_mms = (int)(((int64_t)max_subs * rlen + 50) / 100);
    todo = !(h.ext & (K4_EXT_INDEL | K4_EXT_SPLICE)) && low_mm > max_mms && (uint32_t)h.match_len == rlen && rlen > 0 &&
           h.chrom_id >= 1 && h.chrom_id <= ix.n_entries;
  }
  uint32_t n_fixed = 0;
  bool corrected = false, rejected = false;
  // ---- phase 2: the lanes that stay
  if (todo) {
    const uint64_t first = ix.ent_start[h.chrom_id - 1] + h.match_loci;  // the window on the concatenated sequences
    if (first + rlen - 1 <= ix.ent_end[h.chrom_id - 1]) {                 // (a record that leaves its sequence is left alone)
      const uint32_t k = min((uint32_t)klen, rlen);
      const bool minus = h.strand == '-';
      const uint64_t lo = minus ? first + rlen - k : first;  // the k loci that face the read's first k bases
      // the target symbols, one nibble each, in read order
      uint64_t tn = 0;
      if (!k4d_any_exc(ix, (int64_t)lo, (int64_t)(lo + k))) {
        const uint32_t* p = ix.ref2 + (lo >> 4);
        const uint64_t v = ((((uint64_t)p[0]) << 32) | p[1]) << (2 * (uint32_t)(lo & 15));  // base q of the span: bits 63 - 2q, 62 - 2q
#pragma unroll
        for (int j = 0; j < K4_PRIMER_KLEN; j++) {
          const int q = minus ? (int)k - 1 - j : j;
          uint64_t b = q >= 0 ? (v >> (62 - 2 * q)) & 3u : 0u;
          if (minus) b = 3u - b;
          tn |= b << (4 * j);
        }
      } else {
        K4Tb tb;
        tb.init(ix);
        for (uint32_t j = 0; j < k; j++) {
          uint64_t b = tb.get((int64_t)(minus ? lo + k - 1 - j : lo + j));
          if (minus && b <= 3u) b = 3u - b;  // CSeqTrans::ReverseComplement leaves the other symbols as they are
          tn |= b << (4 * j);
        }
      }
      uint8_t* rd = rs.reads + rs.offs[i];
      uint32_t rb[K4_PRIMER_KLEN];
      uint32_t mm_mask = 0;
#pragma unroll
      for (int j = 0; j < K4_PRIMER_KLEN; j++) {
        rb[j] = (uint32_t)j < k ? rd[j] : 0u;
        if ((uint32_t)j < k && (rb[j] & 7u) != (uint32_t)((tn >> (4 * j)) & 0xFu)) mm_mask |= 1u << j;
      }
      // the first walk (:2175-2182): every mismatch lowers CurMMs, until it is within MaxMMs
      int cur = low_mm;
      uint32_t fix = 0;
      bool within = false;
#pragma unroll
      for (int j = 0; j < K4_PRIMER_KLEN; j++) {
        if (!within && ((mm_mask >> j) & 1u)) {
          fix |= 1u << j;
          within = --cur <= max_mms;
        }
      }
      if (within) {  // the second walk (:2185-2200) rewrites what the first one counted
#pragma unroll
        for (int j = 0; j < K4_PRIMER_KLEN; j++)
          if ((fix >> j) & 1u) rd[j] = (uint8_t)((rb[j] & 0xF8u) | (uint32_t)((tn >> (4 * j)) & 0xFu));
        rs.set_low_mm(i, cur);
        rs.hit_ptr(i)->mismatches = (uint8_t)cur;
        corrected = true;
        n_fixed = (uint32_t)__popc(fix);
      } else {  // NAR and NumHits; LowHitInstances stays (:2202-2207)
        rs.reject(i, K4_NAR_NOHIT, false);
        rejected = true;
      }
    }
  }
  // ---- the totals: wave, block, grid
  const uint32_t w_corr = (uint32_t)__popcll(__ballot(corrected)), w_rej = (uint32_t)__popcll(__ballot(rejected));
  if (w_corr | w_rej) {  // (wave-uniform)
    uint32_t w_fix = n_fixed;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) w_fix += __shfl_xor(w_fix, d, 64);
    if ((threadIdx.x & 63) == 0) {
      if (w_corr) { atomicAdd(&s_tot[0], w_corr); atomicAdd(&s_tot[1], w_fix); }
      if (w_rej) atomicAdd(&s_tot[2], w_rej);
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_tot[threadIdx.x]) atomicAdd(totals + threadIdx.x, (unsigned long long)s_tot[threadIdx.x]);
}

}  // namespace

extern "C" int k4_pcr5_primer_correct_dev(k4_index* ix, int32_t max_subs, int32_t klen, int pe, int64_t n_reads, int32_t max_ml,
                                          void* d_rr_or_pe, void* d_hits, void* d_reads, const void* d_offs, const void* d_lens,
                                          int64_t counts[3], void* stream) {
  if (!ix) return K4_ERR_PARAMS;
  if (counts) counts[0] = counts[1] = counts[2] = 0;
  if (max_subs < 0 || max_subs > 15) return k4_fail(ix, K4_ERR_PARAMS, "substitutions per 100bp %d outside of range 0..15", (int)max_subs);
  if (klen > K4_PRIMER_KLEN) return k4_fail(ix, K4_ERR_PARAMS, "primer correction over %d bases, at most %d", (int)klen, K4_PRIMER_KLEN);
  if (klen < 1 || n_reads <= 0) return K4_OK;  // (KLen < 1: :2138)
  K4ReadSet rs;
  K4_TRY(k4s_read_set(ix, pe, n_reads, d_rr_or_pe, d_hits, max_ml, d_rr_or_pe, nullptr, d_reads, d_offs, d_lens, K4RS_HITS | K4RS_READS, &rs));
  const int64_t blocks = (n_reads + 255) / 256;
  if (blocks > 0x7FFFFFFFll) return k4_fail(ix, K4_ERR_PARAMS, "at most 2^39 reads per call");
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  K4DevBuf cnt;
  K4_HIP(ix, cnt.alloc(8 * 3));
  K4_HIP(ix, hipMemsetAsync(cnt.p, 0, 8 * 3, st));
  hipLaunchKernelGGL(k4k_primer_correct, dim3((unsigned)blocks), dim3(256), 0, st, ix->d, (int)max_subs, (int)klen, rs,
                     cnt.as<unsigned long long>());
  K4_HIP(ix, hipGetLastError());
  unsigned long long c[3];
  K4_TRY(k4s_read_back(ix, &c, cnt.p, st));
  if (counts)
    for (int k = 0; k < 3; k++) counts[k] = (int64_t)c[k];
  return K4_OK;
}
