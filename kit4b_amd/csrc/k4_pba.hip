// kit4b_amd/csrc/k4_pba.hip -- genpba's packed base alleles over device-resident alignments.
//
//   kalignerPBA             ngskit4b/KAlignerCL.cpp:1540-2290   the front end: kalign's Process with eFMPBA, no SAM
//   CKAligner::ProcessSNPs  ngskit4b/KAligner.cpp:8168-8575     per-locus base counts over the accepted alignments of a chromosome
//   CKAligner::OutputSNPs   ngskit4b/KAligner.cpp:7194-7317     its PBA branch: file header, one record per chromosome, the WIG feed
//
// Device: the pile-up SNP calling uses (k4_pileup.h), then ONE streaming pass over the seven count arrays that writes the PBA byte and
// the N-excluded coverage of every locus and finds the coverage's maximum (k4k_pba_classify; the rule itself is k4_pba_classify.h).
// The pass writes the coverage as one saturated byte per locus -- whole-genome coverage fits a byte -- and only a chromosome whose
// maximum does not fit runs a second, narrower pass into 2 or 4 bytes per locus (k4k_pba_coverage).
// Host: the bytes and the coverage come down per chromosome; the WIG walk runs on a host thread per chromosome while the device
// works on the next one.  The download itself is waited for before the next chromosome's memset is queued (one stream, one set of
// count arrays): the device work of chromosome c + 1 does not overlap the download of chromosome c.
// K4_PBA_TIMES=<file>: one line per chromosome with the milliseconds of its memset, pile-up, classification pass, wider coverage
// pass, downloads and WIG walk is appended there (tools/pba_bench.py); it adds three events and nothing else to the stream.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include "k4_device.h"
#include "k4_pba_classify.h"
#include "k4_pileup.h"
#include "k4_stage.h"

namespace {

#define K4_PBA_LPT 4  // loci per thread: one 16-byte load per count array, one 4-byte store of PBA bytes and one of coverage bytes

// the target's symbols at pos .. pos + 3; `n` of them lie inside the chromosome (the others: 4, which matches no allele)
K4_DEV void pba_ref_bases(const K4DevIndex& ix, uint64_t pos, uint32_t n, uint32_t (&rb)[K4_PBA_LPT]) {
  const uint64_t blk = pos >> K4_EXC_SHIFT;
  // all four in one packed word of a block without a non-ACGT symbol: one bitmap word and one sequence word for the thread
  if (n == K4_PBA_LPT && (pos & 15) <= 16 - K4_PBA_LPT && !((ix.excbm[blk >> 5] >> (blk & 31)) & 1)) {
    const uint32_t w = ix.ref2[pos >> 4];
#pragma unroll
    for (uint32_t j = 0; j < K4_PBA_LPT; j++) rb[j] = (w >> (30 - 2 * ((uint32_t)(pos & 15) + j))) & 3;
    return;
  }
#pragma unroll
  for (uint32_t j = 0; j < K4_PBA_LPT; j++) rb[j] = j < n ? k4d_ref_base(ix, pos + j) : 4u;
}

// OutputSNPs' PBA loop (:7262-7302) over a chromosome: thread t takes the loci [4 t, 4 t + 4).  The count arrays are read with
// 16-byte loads (a wave reads 1 KiB in a row of each of the seven; the arrays start at a 4-byte boundary, which is all gfx950 asks
// of a wide load, and carry 16 zeroed words behind the chromosome, so the last thread's load stays inside them); pba and cov8 get
// one 4-byte store each, the last thread of a chromosome whose length is no multiple of four writes its 1..3 bytes one by one.
__global__ void __launch_bounds__(256) k4k_pba_classify(SnpArgs a, uint8_t* __restrict__ pba, uint8_t* __restrict__ cov8, uint32_t* __restrict__ mx) {
  const uint64_t l0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * K4_PBA_LPT;
  uint32_t m = 0;
  if (l0 < a.clen) {
    const size_t S = K4_SNP_STRIDE(a);
    const uint32_t n = (uint32_t)min((uint64_t)K4_PBA_LPT, (uint64_t)a.clen - l0);
    uint32_t c[7][K4_PBA_LPT], rb[K4_PBA_LPT];
#pragma unroll
    for (int k = 0; k < 7; k++) k4d_load_words<K4_PBA_LPT>(a.cnt + k * S + l0, c[k]);
    pba_ref_bases(a.ix, a.cs + l0, n, rb);
    uint32_t pw = 0, cw = 0;
#pragma unroll
    for (int j = 0; j < K4_PBA_LPT; j++) {
      const uint32_t by_base[5] = {c[2][j], c[3][j], c[4][j], c[5][j], c[6][j]};
      uint32_t cov;
      const uint32_t b = k4_pba_byte(c[0][j], c[1][j], by_base, rb[j], &cov);
      m = max(m, cov);
      pw |= b << (8 * j);
      cw |= min(cov, 255u) << (8 * j);
    }
    if (n == K4_PBA_LPT) {
      *reinterpret_cast<uint32_t*>(pba + l0) = pw;
      *reinterpret_cast<uint32_t*>(cov8 + l0) = cw;
    } else
      for (uint32_t j = 0; j < n; j++) { pba[l0 + j] = (uint8_t)(pw >> (8 * j)); cov8[l0 + j] = (uint8_t)(cw >> (8 * j)); }
  }
  for (int d = 32; d > 0; d >>= 1) m = max(m, (uint32_t)__shfl_down(m, d, 64));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(mx, m);
}

// the coverage of a chromosome whose maximum does not fit a byte, in 2 or 4 bytes per locus: four loci per thread as above, one
// 8- or 16-byte store (the buffer is 256-byte aligned and 4 t * sizeof(T) a multiple of the store's size)
template <typename T>
__global__ void __launch_bounds__(256) k4k_pba_coverage(SnpArgs a, T* __restrict__ cov) {
  const uint64_t l0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * K4_PBA_LPT;
  if (l0 >= a.clen) return;
  const size_t S = K4_SNP_STRIDE(a);
  const uint32_t n = (uint32_t)min((uint64_t)K4_PBA_LPT, (uint64_t)a.clen - l0);
  uint32_t ref[K4_PBA_LPT], non[K4_PBA_LPT], nn[K4_PBA_LPT];
  k4d_load_words<K4_PBA_LPT>(a.cnt + l0, ref);
  k4d_load_words<K4_PBA_LPT>(a.cnt + S + l0, non);
  k4d_load_words<K4_PBA_LPT>(a.cnt + 6 * S + l0, nn);
  typedef T Vec __attribute__((ext_vector_type(K4_PBA_LPT)));
  Vec v;
#pragma unroll
  for (int j = 0; j < K4_PBA_LPT; j++) v[j] = (T)(non[j] + ref[j] - nn[j]);
  if (n == K4_PBA_LPT) *reinterpret_cast<Vec*>(cov + l0) = v;
  else
    for (uint32_t j = 0; j < n; j++) cov[l0 + j] = v[j];
}

}  // namespace

// the record of a sequence (:7254-7259): name length, name, NUL, sequence length, then room for the bytes; returns where they start
static size_t pba_record(std::vector<std::vector<uint8_t>>& recs, const char* name, uint32_t clen) {
  const size_t nl = std::min<size_t>(strlen(name), 255), head = 1 + nl + 1 + 4;
  recs.emplace_back(head + (size_t)clen);
  std::vector<uint8_t>& rec = recs.back();
  rec[0] = (uint8_t)nl;
  memcpy(&rec[1], name, nl);
  for (int k = 0; k < 4; k++) rec[2 + nl + k] = (uint8_t)(clen >> (8 * k));
  return head;
}

// CUtility::TrimQuotedWhitespcExtd + ReduceWhitespace are the front end's business (k4align); the ids arrive here as they are written
extern "C" int k4_pba_run_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml, const void* d_pe,
                              const void* d_reads, const void* d_offs, const void* d_lens, const char* experiment_id, const char* readset_id,
                              k4_pba_files* out, void* stream) {
  if (!ix || !out) return K4_ERR_PARAMS;
  K4HandOut hand(out);
  if (n_units < 0 || !experiment_id || !readset_id) return k4_fail(ix, K4_ERR_PARAMS, "packed base alleles: parameters out of range");
  const char* times_path = getenv("K4_PBA_TIMES");
  FILE* times = times_path && *times_path ? fopen(times_path, "a") : nullptr;
  std::unique_ptr<FILE, int (*)(FILE*)> times_close(times, fclose);
  WigQueue wig;  // (behind the trace file: the walks are waited for before it closes)
  wig.trace = times;
  PileupWalk w;
  K4_TRY(w.open(ix, K4Records{pe, n_units, d_rr, d_hits, max_ml, d_pe, d_reads, d_offs, d_lens}, stream, times != nullptr));
  hipStream_t st = w.st;
  const SnpArgs& a = w.a;
  K4DevBuf pbab, covb, covmax;
  // :7224: the header once, a NUL behind it; the records follow
  std::vector<std::vector<uint8_t>> recs;  // one per chromosome with alignments, in chromosome order
  const std::string hdr = std::string("Type:PbA\nVersion:1\nExperimentID:") + experiment_id + "\nReferenceID:" + ix->dataset + "\nReadsetID:" + readset_id;
  auto ms_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
  for (bool got = false;;) {
    K4_TRY(w.next(&got));
    if (!got) break;
    if (!pbab.p) {
      K4_HIP(ix, pbab.alloc(w.S));
      K4_HIP(ix, covb.alloc(w.S * 4));
      K4_HIP(ix, covmax.alloc(4));
    }
    K4_HIP(ix, hipMemsetAsync(covmax.p, 0, 4, st));
    const dim3 grid((unsigned)(((uint64_t)a.clen + 256 * K4_PBA_LPT - 1) / (256 * K4_PBA_LPT)));
    auto t_cls = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(k4k_pba_classify, grid, dim3(256), 0, st, a, pbab.as<uint8_t>(), covb.as<uint8_t>(), covmax.as<uint32_t>());
    K4_HIP(ix, hipGetLastError());
    uint32_t mx = 0;
    K4_TRY(k4s_read_back(ix, &mx, covmax.p, st));
    const double ms_classify = ms_since(t_cls);
    const size_t head = pba_record(recs, w.e->name, a.clen);
    const int width = mx < 256 ? 1 : mx < 65536 ? 2 : 4;
    auto t_wide = std::chrono::steady_clock::now();
    if (width == 2) hipLaunchKernelGGL(k4k_pba_coverage<uint16_t>, grid, dim3(256), 0, st, a, covb.as<uint16_t>());
    else if (width == 4) hipLaunchKernelGGL(k4k_pba_coverage<uint32_t>, grid, dim3(256), 0, st, a, covb.as<uint32_t>());
    K4_HIP(ix, hipGetLastError());
    if (times && width > 1) K4_HIP(ix, hipStreamSynchronize(st));
    const double ms_wide = width > 1 ? ms_since(t_wide) : 0.0;
    auto t_down = std::chrono::steady_clock::now();
    K4_HIP(ix, hipMemcpyAsync(recs.back().data() + head, pbab.p, a.clen, hipMemcpyDeviceToHost, st));
    // no track line (:8192), the loci counted from 1, every chromosome's open span closed at its end (:7303)
    K4_TRY(wig.add(ix, st, covb.p, width, a.clen, w.e->name, 1u, true));
    const double ms_down = ms_since(t_down);
    if (times)
      fprintf(times, "chrom %s len %u reads %llu max_cov %u width %d memset_ms %.3f pileup_ms %.3f classify_ms %.3f wide_ms %.3f download_ms %.3f\n", w.e->name,
              a.clen, w.t[2], mx, width, w.ms_memset, w.ms_pileup, ms_classify, ms_wide, ms_down);
  }
  size_t pba_total = recs.empty() ? 0 : hdr.size() + 1;  // (the header is written with the first chromosome: no chromosome, an empty file)
  for (const std::vector<uint8_t>& r : recs) pba_total += r.size();
  K4_TRY(hand.block(ix, &out->pba, &out->pba_bytes, pba_total));
  size_t at = 0;
  if (!recs.empty()) { memcpy(out->pba, hdr.c_str(), hdr.size() + 1); at = hdr.size() + 1; }
  for (const std::vector<uint8_t>& r : recs) { memcpy(out->pba + at, r.data(), r.size()); at += r.size(); }
  K4_TRY(wig.finish(ix, nullptr, hand, &out->wig, &out->wig_bytes));
  out->n_chroms = recs.size();
  return hand.ok();
}

// the rule alone, on the host: no device, no index.  cnt7: seven arrays of `stride` words each (ref, nonref, A, C, G, T, N), as the
// pile-up leaves them; ref_bases: the target's symbol per locus
extern "C" int k4_pba_classify_host(const uint32_t* cnt7, uint64_t stride, uint32_t n_loci, const uint8_t* ref_bases, uint8_t* pba, uint32_t* coverage) {
  if ((!cnt7 || !ref_bases || !pba || !coverage) && n_loci) return K4_ERR_PARAMS;
  if (stride < n_loci) return K4_ERR_PARAMS;
  for (uint32_t l = 0; l < n_loci; l++) {
    const uint32_t by_base[5] = {cnt7[2 * stride + l], cnt7[3 * stride + l], cnt7[4 * stride + l], cnt7[5 * stride + l], cnt7[6 * stride + l]};
    pba[l] = k4_pba_byte(cnt7[l], cnt7[stride + l], by_base, ref_bases[l], &coverage[l]);
  }
  return K4_OK;
}
