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
#include <future>
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

// CUtility::TrimQuotedWhitespcExtd + ReduceWhitespace are the front end's business (k4align); the ids arrive here as they are written
extern "C" int k4_pba_run_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml, const void* d_pe,
                              const void* d_reads, const void* d_offs, const void* d_lens, const char* experiment_id, const char* readset_id,
                              k4_pba_files* out, void* stream) {
  if (!ix || !out) return K4_ERR_PARAMS;
  memset(out, 0, sizeof(*out));
  if (n_units < 0 || !experiment_id || !readset_id) return k4_fail(ix, K4_ERR_PARAMS, "packed base alleles: parameters out of range");
  SnpArgs a;
  memset(&a, 0, sizeof(a));
  a.ix = ix->d;
  K4_TRY(k4s_read_set(ix, pe, n_units, d_rr, d_hits, max_ml, d_pe, nullptr, d_reads, d_offs, d_lens, K4RS_HITS | K4RS_READS | K4RS_UNITS, &a.rs));
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t max_len = 0;
  for (const k4_entry& e : ix->entries) max_len = std::max(max_len, e.seq_len);
  const size_t S = (size_t)max_len + 16;
  std::vector<uint8_t> chrom_hit((size_t)ix->d.n_entries + 1, 0);
  std::vector<uint64_t> ent_start_h((size_t)ix->d.n_entries, 0);
  K4DevBuf cnt, tot, pbab, covb, covmax;
  if (a.rs.n_reads > 0 && ix->d.n_entries) {
    K4DevBuf flags;
    K4_HIP(ix, flags.alloc(chrom_hit.size()));
    K4_HIP(ix, hipMemsetAsync(flags.p, 0, chrom_hit.size(), st));
    hipLaunchKernelGGL(k4k_snp_mark, dim3((unsigned)std::min<int64_t>((a.rs.n_reads + 255) / 256, 2048)), dim3(256), 0, st, a, flags.as<uint8_t>(), ix->d.n_entries);
    K4_HIP(ix, hipMemcpyAsync(chrom_hit.data(), flags.p, chrom_hit.size(), hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipMemcpyAsync(ent_start_h.data(), ix->ent_start.p, ent_start_h.size() * 8, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipStreamSynchronize(st));
  }
  // :7224: the header once, a NUL behind it; the records follow
  std::vector<std::vector<uint8_t>> recs;  // one per chromosome with alignments, in chromosome order
  std::string hdr = std::string("Type:PbA\nVersion:1\nExperimentID:") + experiment_id + "\nReferenceID:" + ix->dataset + "\nReadsetID:" + readset_id;
  const char* times_path = getenv("K4_PBA_TIMES");
  FILE* times = times_path && *times_path ? fopen(times_path, "a") : nullptr;
  std::unique_ptr<FILE, int (*)(FILE*)> times_close(times, fclose);
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  if (times)
    for (hipEvent_t& e : ev) K4_HIP(ix, hipEventCreate(&e));
  struct EvGuard { hipEvent_t* ev; ~EvGuard() { for (int k = 0; k < 3; k++) if (ev[k]) (void)hipEventDestroy(ev[k]); } } ev_guard{ev};
  std::vector<std::future<WigOut>> wig_jobs;  // (behind the trace file: the walks are waited for before it closes)
  auto ms_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
  for (uint32_t chrom = 1; chrom <= ix->d.n_entries && a.rs.n_reads > 0; chrom++) {
    if (!chrom_hit[chrom]) continue;
    if (!cnt.p) {
      K4_HIP(ix, cnt.alloc(7 * S * 4));
      K4_HIP(ix, tot.alloc(4 * 8));
      K4_HIP(ix, pbab.alloc(S));
      K4_HIP(ix, covb.alloc(S * 4));
      K4_HIP(ix, covmax.alloc(4));
    }
    const k4_entry& e = ix->entries[chrom - 1];
    a.chrom_id = chrom; a.clen = e.seq_len; a.cnt = cnt.as<uint32_t>(); a.tot = tot.as<unsigned long long>();
    a.cs = ent_start_h[chrom - 1];
    const size_t Sc = K4_SNP_STRIDE(a);
    if (times) K4_HIP(ix, hipEventRecord(ev[0], st));
    K4_HIP(ix, hipMemsetAsync(cnt.p, 0, 7 * Sc * 4, st));
    K4_HIP(ix, hipMemsetAsync(tot.p, 0, 32, st));
    K4_HIP(ix, hipMemsetAsync(covmax.p, 0, 4, st));
    if (times) K4_HIP(ix, hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(k4k_snp_pileup, dim3(2048), dim3(256), 0, st, a);
    if (times) K4_HIP(ix, hipEventRecord(ev[2], st));
    unsigned long long t3[4] = {0, 0, 0, 0};
    K4_TRY(k4s_read_back(ix, &t3, tot.p, st));
    float ms_memset = 0, ms_pileup = 0;
    if (times) { K4_HIP(ix, hipEventElapsedTime(&ms_memset, ev[0], ev[1])); K4_HIP(ix, hipEventElapsedTime(&ms_pileup, ev[1], ev[2])); }
    if (t3[2] == 0) continue;  // no alignment on this chromosome: no record (the reference never gets to OutputSNPs for it)
    const dim3 grid((unsigned)(((uint64_t)a.clen + 256 * K4_PBA_LPT - 1) / (256 * K4_PBA_LPT)));
    auto t_cls = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(k4k_pba_classify, grid, dim3(256), 0, st, a, pbab.as<uint8_t>(), covb.as<uint8_t>(), covmax.as<uint32_t>());
    K4_HIP(ix, hipGetLastError());
    uint32_t mx = 0;
    K4_TRY(k4s_read_back(ix, &mx, covmax.p, st));
    const double ms_classify = ms_since(t_cls);
    // the record (:7254-7259): name length, name, NUL, sequence length, then the bytes straight from the device
    const size_t nl = std::min<size_t>(strlen(e.name), 255), head = 1 + nl + 1 + 4;
    recs.emplace_back(head + (size_t)a.clen);
    std::vector<uint8_t>& rec = recs.back();
    rec[0] = (uint8_t)nl;
    memcpy(&rec[1], e.name, nl);
    rec[1 + nl] = 0;
    for (int k = 0; k < 4; k++) rec[2 + nl + k] = (uint8_t)(a.clen >> (8 * k));
    const int width = mx < 256 ? 1 : mx < 65536 ? 2 : 4;
    auto t_wide = std::chrono::steady_clock::now();
    if (width == 2) hipLaunchKernelGGL(k4k_pba_coverage<uint16_t>, grid, dim3(256), 0, st, a, covb.as<uint16_t>());
    else if (width == 4) hipLaunchKernelGGL(k4k_pba_coverage<uint32_t>, grid, dim3(256), 0, st, a, covb.as<uint32_t>());
    if (times && width > 1) K4_HIP(ix, hipStreamSynchronize(st));
    const double ms_wide = width > 1 ? ms_since(t_wide) : 0.0;
    auto t_down = std::chrono::steady_clock::now();
    K4_HIP(ix, hipMemcpyAsync(rec.data() + head, pbab.p, a.clen, hipMemcpyDeviceToHost, st));
    std::unique_ptr<uint8_t[]> cov(new uint8_t[((size_t)a.clen + 1) * (size_t)width]);
    K4_HIP(ix, hipMemcpyAsync(cov.get(), covb.p, (size_t)a.clen * (size_t)width, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipStreamSynchronize(st));
    const double ms_down = ms_since(t_down);
    if (wig_jobs.size() >= 12) wig_jobs[wig_jobs.size() - 12].wait();  // (at most twelve chromosomes' walks in flight)
    wig_jobs.push_back(std::async(std::launch::async, [times](std::unique_ptr<uint8_t[]> c, int w, uint32_t n, std::string nm) {
      auto t0 = std::chrono::steady_clock::now();
      WigOut o = wig_chromosome(std::move(c), w, n, std::move(nm), 1u);
      if (times) {  // (the walks of several chromosomes run side by side: each line is written whole)
        char line[160];
        const int k = snprintf(line, sizeof(line), "walk %u %.3f\n", n, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        fwrite(line, 1, (size_t)k, times);
      }
      return o;
    }, std::move(cov), width, a.clen, std::string(e.name)));
    if (times)
      fprintf(times, "chrom %s len %u reads %llu max_cov %u width %d memset_ms %.3f pileup_ms %.3f classify_ms %.3f wide_ms %.3f download_ms %.3f\n", e.name,
              a.clen, t3[2], mx, width, ms_memset, ms_pileup, ms_classify, ms_wide, ms_down);
  }
  // no track line (:8192), every chromosome's open span closed at its end (:7303)
  std::vector<WigOut> parts;
  parts.reserve(wig_jobs.size());
  size_t wig_total = 0;
  for (std::future<WigOut>& f : wig_jobs) {
    parts.push_back(f.get());
    wig_total += parts.back().body.size() + parts.back().tail.size();
  }
  size_t pba_total = 0;
  for (const std::vector<uint8_t>& r : recs) pba_total += r.size();
  if (!recs.empty()) pba_total += hdr.size() + 1;  // (the header is written with the first chromosome: no chromosome, an empty file)
  uint8_t* po = (uint8_t*)malloc(pba_total + 1);
  char* wo = (char*)malloc(wig_total + 1);
  if (!po || !wo) { free(po); free(wo); return k4_fail(ix, K4_ERR_MEM, "out of memory"); }
  size_t at = 0;
  if (!recs.empty()) { memcpy(po, hdr.c_str(), hdr.size() + 1); at = hdr.size() + 1; }
  for (const std::vector<uint8_t>& r : recs) { memcpy(po + at, r.data(), r.size()); at += r.size(); }
  po[at] = 0;
  at = 0;
  for (const WigOut& w : parts) {
    memcpy(wo + at, w.body.data(), w.body.size()); at += w.body.size();
    memcpy(wo + at, w.tail.data(), w.tail.size()); at += w.tail.size();
  }
  wo[at] = 0;
  out->pba = po; out->pba_bytes = pba_total;
  out->wig = wo; out->wig_bytes = wig_total;
  out->n_chroms = recs.size();
  return K4_OK;
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
