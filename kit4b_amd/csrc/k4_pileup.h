// kit4b_amd/csrc/k4_pileup.h -- what the two readers of CKAligner::ProcessSNPs' per-locus base counts share: SNP calling
// (k4_snp.hip) and the packed base alleles of genpba (k4_pba.hip).  Device: the pile-up of a chromosome's accepted alignments into
// seven count arrays and the pass that tells which sequences have any.  Host: the walk over the sequences with piled-up alignments
// (PileupWalk), the queue of the coverage WIG's per-chromosome walks (WigQueue, wig_walk) and the hand-out of host blocks to an
// entry point's caller (K4HandOut).
// Everything sits in the including file's anonymous namespace: each of the two translation units compiles its own kernels.
#pragma once
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <future>
#include <memory>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include "k4_device.h"
#include "k4_stage.h"

namespace {

struct SnpArgs {
  K4DevIndex ix;
  K4ReadSet rs;      // (read only: no kernel of the two files writes a record)
  uint32_t chrom_id;
  uint64_t cs;       // concat offset of the chromosome
  uint32_t clen;
  uint32_t* cnt;     // seven arrays of clen + 16: ref, nonref, A, C, G, T, N
  unsigned long long* tot;  // [0] TotMatch [1] TotMismatch [2] reads piled up [3] their aligned bases
};
#define K4_SNP_STRIDE(a) ((size_t)(a).clen + 16)

// ProcessSNPs' inner loop (:8468-8557, base space), one wave per accepted alignment on this chromosome
__global__ void __launch_bounds__(256) k4k_snp_pileup(SnpArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * 256) >> 6;
  unsigned long long m = 0, mm = 0, nr = 0, nb = 0;
  for (int64_t i = wave0; i < a.rs.n_reads; i += n_waves) {
    if (a.rs.nar(i) != K4_NAR_ACCEPTED) continue;
    const k4_hit h = a.rs.hit(i);
    if (h.chrom_id != a.chrom_id || (h.ext & (K4_EXT_INDEL | K4_EXT_SPLICE))) continue;
    const uint32_t tl = K4_HIT_TRIM_LEFT(h);
    uint32_t match_len = k4d_adj_len(h);
    const uint32_t loci0 = k4d_adj_start(h);
    if ((uint64_t)loci0 + match_len > a.clen) continue;                  // (GetSeq comes back short: the read is skipped, :8420)
    const uint8_t* src = a.rs.reads + a.rs.offs[i] + tl;
    if (lane == 0) { nr++; nb += match_len; }
    for (uint32_t q = lane; q < match_len; q += 64) {
      const uint32_t ref = k4d_ref_base(a.ix, a.cs + loci0 + q);
      uint32_t r = h.strand == '+' ? (src[q] & 7u) : (src[match_len - 1 - q] & 7u);
      if (h.strand != '+' && r <= 3) r = 3 - r;
      if (ref >= 4 || r > 4) continue;
      uint32_t* c = a.cnt + loci0 + q;
      if (ref == r) { atomicAdd(c, 1u); m++; }
      else {
        atomicAdd(c + K4_SNP_STRIDE(a), 1u);
        atomicAdd(c + (2 + r) * K4_SNP_STRIDE(a), 1u);
        mm++;
      }
    }
  }
  for (int d = 32; d > 0; d >>= 1) { m += __shfl_down(m, d, 64); mm += __shfl_down(mm, d, 64); }
  if (lane == 0) {
    if (m) atomicAdd(&a.tot[0], m);
    if (mm) atomicAdd(&a.tot[1], mm);
    if (nr) { atomicAdd(&a.tot[2], nr); atomicAdd(&a.tot[3], nb); }
  }
}

// which sequences hold an alignment the pile-up would take at all: one pass over the reads before the per-sequence work, so that
// an assembly of 10^5 contigs costs its hit contigs, not its contigs (the reference walks its sorted reads once)
__global__ void __launch_bounds__(256) k4k_snp_mark(SnpArgs a, uint8_t* __restrict__ flags, uint32_t n_entries) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.rs.n_reads; i += stride) {
    if (a.rs.nar(i) != K4_NAR_ACCEPTED) continue;
    const k4_hit h = a.rs.hit(i);
    if ((h.ext & (K4_EXT_INDEL | K4_EXT_SPLICE)) || h.chrom_id < 1 || h.chrom_id > n_entries) continue;
    flags[h.chrom_id] = 1;
  }
}

// The coverage WIG kalign writes beside the SNP file and genpba beside the .pba file: variableStep spans of roughly equal coverage
// (AccumWIGCnts / CompleteWIGSpan, KAligner.cpp:6993-7085).  SNP calling feeds the locus counted from 0 (:7375) -- so a span that
// starts at locus 0 is never written -- and genpba counted from 1 (:7267): `first` is the number of the chromosome's first locus.
// The walk is sequential by nature (where a span ends depends on its running mean): one host thread per chromosome, running while
// the device piles up the next chromosomes.  Returns the text of the chromosome's closed spans; `tail` = what closing the last open
// span adds (SNP calling does that only for chromosomes with at least one candidate locus, :7582-7608 / :8135; genpba always, :7303).
struct WigOut { std::string body, tail; };
// The running mean cnts / len is kept as quotient and remainder (a span grows by one locus at a time), so the walk has no division:
// 100 * (cnts / len) against 100 c, 75 c and 125 c is q against c, 4 q against 3 c and 5 c.
template <typename T>
static WigOut wig_walk(const T* cov, uint32_t clen, const std::string& name, uint32_t first) {
  WigOut o;
  uint32_t loci = 0, len = 0, rptd_len = 0;
  bool started = false, rptd = false;  // m_WIGChromID != 0, m_WIGRptdChromID == this chromosome
  uint64_t cnts = 0, q = 0;            // q = cnts / len
  int64_t r = 0;                       // cnts - q * len
  // (a genome at low coverage makes a span of nearly every run of equal coverage -- hundreds of millions of lines: own digits, no printf)
  const std::string head = "variableStep chrom=" + name + " span=";
  char line[64];
  auto put = [](char* p, uint32_t v) {
    char t[10];
    int n = 0;
    do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) *p++ = t[--n];
    return p;
  };
  auto complete = [&](std::string& dst) {
    if (started && len > 0 && loci > 0 && cnts > 0) {
      if (!rptd || len != rptd_len) {
        dst += head;
        char* p = put(line, len);
        *p++ = '\n';
        dst.append(line, (size_t)(p - line));
        rptd = true; rptd_len = len;
      }
      char* p = put(line, loci);
      *p++ = ' ';
      p = put(p, (uint32_t)(q + (r > 0 ? 1 : 0)));  // (cnts + len - 1) / len
      *p++ = '\n';
      dst.append(line, (size_t)(p - line));
    }
    loci = 0; len = 0; cnts = 0;
  };
  for (uint32_t l = 0; l < clen; l++) {
    const uint64_t c = cov[l];
    if (!started || len >= 100000u || c == 0) {
      if (started) complete(o.body);
      if (c > 0) { started = true; loci = l + first; len = 1; cnts = c; q = c; r = 0; }
      continue;
    }
    if (len == 0 || cnts == 0) { loci = l + first; len = 1; cnts = c; q = c; r = 0; continue; }
    if ((c <= 5 && c != q) || 4 * q < 3 * c || 4 * q >= 5 * c) {
      complete(o.body);
      loci = l + first; len = 1; cnts = c; q = c; r = 0;
      continue;
    }
    cnts += c;
    len = l + first - loci + 1;  // (= len + 1: the loci of a span follow each other)
    r += (int64_t)c - (int64_t)q;
    while (r >= (int64_t)len) { q++; r -= len; }
    while (r < 0) { q--; r += len; }
  }
  complete(o.tail);
  return o;
}
// `width` bytes per locus (k4k_snp_coverage, k4k_pba_coverage)
static WigOut wig_chromosome(std::unique_ptr<uint8_t[]> cov, int width, uint32_t clen, std::string name, uint32_t first) {
  if (width == 1) return wig_walk<uint8_t>(cov.get(), clen, name, first);
  if (width == 2) return wig_walk<uint16_t>((const uint16_t*)cov.get(), clen, name, first);
  return wig_walk<uint32_t>((const uint32_t*)cov.get(), clen, name, first);
}

// The record arguments of a C ABI entry point as they came: what an entry point passes on instead of nine parameters.
struct K4Records { int pe; int64_t n_units; const void *d_rr, *d_hits; int32_t max_ml; const void *d_pe, *d_reads, *d_offs, *d_lens; };

// The sorted reads, one sequence after the other: open() makes the view of the records, sizes the count arrays for the longest
// sequence and brings down which sequences hold an alignment the pile-up would take (k4k_snp_mark) -- nothing the pile-up would
// take, no device work and no synchronisation for that sequence.  next() hands out each sequence with at least one piled-up
// alignment: its counts are zeroed and piled up on the stream and the four totals are on the host (the reference never gets to
// OutputSNPs for a sequence without one).  The count arrays are allocated with the first flagged sequence.
struct PileupWalk {
  k4_index* ix = nullptr;
  hipStream_t st = nullptr;
  SnpArgs a;                           // of the sequence handed out last
  const k4_entry* e = nullptr;         // that sequence
  unsigned long long t[4] = {0, 0, 0, 0};  // its totals, as SnpArgs::tot
  size_t S = 0;                        // words per count array for the longest sequence
  K4DevBuf cnt, tot, flags;
  std::vector<uint8_t> hit;            // per chrom_id: flagged
  std::vector<uint64_t> ent_start;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // timed: before the memsets, behind them, behind the pile-up
  float ms_memset = 0, ms_pileup = 0;  // timed: of the sequence handed out last
  ~PileupWalk() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }

  int open(k4_index* ix_, const K4Records& r, void* stream, bool timed = false) {
    ix = ix_;
    st = (hipStream_t)stream;
    memset(&a, 0, sizeof(a));
    a.ix = ix->d;
    K4_TRY(k4s_read_set(ix, r.pe, r.n_units, r.d_rr, r.d_hits, r.max_ml, r.d_pe, nullptr, r.d_reads, r.d_offs, r.d_lens, K4RS_HITS | K4RS_READS | K4RS_UNITS, &a.rs));
    K4_HIP(ix, hipSetDevice(ix->device));
    uint32_t max_len = 0;
    for (const k4_entry& x : ix->entries) max_len = std::max(max_len, x.seq_len);
    S = (size_t)max_len + 16;
    hit.assign((size_t)ix->d.n_entries + 1, 0);
    ent_start.assign((size_t)ix->d.n_entries, 0);
    if (timed)
      for (hipEvent_t& x : ev) K4_HIP(ix, hipEventCreate(&x));
    if (a.rs.n_reads <= 0 || !ix->d.n_entries) return K4_OK;
    K4_HIP(ix, flags.alloc(hit.size()));
    K4_HIP(ix, hipMemsetAsync(flags.p, 0, hit.size(), st));
    hipLaunchKernelGGL(k4k_snp_mark, dim3((unsigned)std::min<int64_t>((a.rs.n_reads + 255) / 256, 2048)), dim3(256), 0, st, a, flags.as<uint8_t>(), ix->d.n_entries);
    K4_HIP(ix, hipGetLastError());
    K4_HIP(ix, hipMemcpyAsync(hit.data(), flags.p, hit.size(), hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipMemcpyAsync(ent_start.data(), ix->ent_start.p, ent_start.size() * 8, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipStreamSynchronize(st));
    return K4_OK;
  }
  int next(bool* got) {
    *got = false;
    while (a.rs.n_reads > 0 && a.chrom_id < ix->d.n_entries) {
      const uint32_t chrom = ++a.chrom_id;
      if (!hit[chrom]) continue;
      if (!cnt.p) {
        K4_HIP(ix, cnt.alloc(7 * S * 4));
        K4_HIP(ix, tot.alloc(4 * 8));
      }
      e = &ix->entries[chrom - 1];
      a.clen = e->seq_len; a.cnt = cnt.as<uint32_t>(); a.tot = tot.as<unsigned long long>();
      a.cs = ent_start[chrom - 1];
      if (ev[0]) K4_HIP(ix, hipEventRecord(ev[0], st));
      K4_HIP(ix, hipMemsetAsync(cnt.p, 0, 7 * K4_SNP_STRIDE(a) * 4, st));
      K4_HIP(ix, hipMemsetAsync(tot.p, 0, 32, st));
      if (ev[0]) K4_HIP(ix, hipEventRecord(ev[1], st));
      hipLaunchKernelGGL(k4k_snp_pileup, dim3(2048), dim3(256), 0, st, a);
      K4_HIP(ix, hipGetLastError());
      if (ev[0]) K4_HIP(ix, hipEventRecord(ev[2], st));
      K4_TRY(k4s_read_back(ix, &t, tot.p, st));
      if (ev[0]) { K4_HIP(ix, hipEventElapsedTime(&ms_memset, ev[0], ev[1])); K4_HIP(ix, hipEventElapsedTime(&ms_pileup, ev[1], ev[2])); }
      if (t[2] == 0) continue;  // no alignment on this sequence
      *got = true;
      return K4_OK;
    }
    return K4_OK;
  }
};

// What an entry point hands to its caller: malloc'd blocks (k4_free_host) in the caller's struct `out`.  The struct is zeroed when
// the guard is made; unless the entry point ends with ok(), the guard frees every block handed out so far and zeroes the struct
// again, so an error never leaves with a live pointer or a lost block.
struct K4HandOut {
  void* out;
  size_t out_bytes;
  std::vector<void*> given;
  bool done = false;
  template <typename Files>
  explicit K4HandOut(Files* o) : out(o), out_bytes(sizeof(Files)) { memset(out, 0, out_bytes); }
  K4HandOut(const K4HandOut&) = delete;
  ~K4HandOut() {
    if (done) return;
    for (void* p : given) free(p);
    memset(out, 0, out_bytes);
  }
  int ok() { done = true; return K4_OK; }
  // a block of `n` bytes for the caller to fill, a NUL behind them
  template <typename P>
  int block(k4_index* ix, P** p, uint64_t* bytes, size_t n) {
    *p = (P*)malloc(n + 1);
    if (!*p) return k4_fail(ix, K4_ERR_MEM, "out of memory");
    given.push_back(*p);
    ((char*)*p)[n] = 0;
    *bytes = n;
    return K4_OK;
  }
  // a text as a block of its own
  int give(k4_index* ix, char** p, uint64_t* bytes, const std::string& s) {
    K4_TRY(block(ix, p, bytes, s.size()));
    memcpy(*p, s.data(), s.size());
    return K4_OK;
  }
};

// The WIG of a run: add() brings a sequence's coverage (`width` bytes per locus) down into a block of its own, waits for the stream
// and starts the sequence's walk on a host thread, at most twelve in flight; finish() gives back the optional header and the
// sequences' texts in one block of the hand-out.  A sequence's tail goes in where `close_tail` says so.
struct WigQueue {
  struct Job { std::future<WigOut> f; bool close_tail; };
  std::vector<Job> jobs;  // one per sequence with alignments, in sequence order
  FILE* trace = nullptr;  // K4_PBA_TIMES: every walk appends "walk <clen> <ms>" (the file must outlive the queue)

  int add(k4_index* ix, hipStream_t st, const void* d_cov, int width, uint32_t clen, const char* name, uint32_t first, bool close_tail, size_t* slot = nullptr) {
    std::unique_ptr<uint8_t[]> cov(new uint8_t[((size_t)clen + 1) * (size_t)width]);
    K4_HIP(ix, hipMemcpyAsync(cov.get(), d_cov, (size_t)clen * (size_t)width, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipStreamSynchronize(st));
    if (jobs.size() >= 12) jobs[jobs.size() - 12].f.wait();
    if (slot) *slot = jobs.size();
    FILE* times = trace;
    jobs.push_back({std::async(std::launch::async, [times, width, clen, first](std::unique_ptr<uint8_t[]> c, std::string nm) {
      auto t0 = std::chrono::steady_clock::now();
      WigOut o = wig_chromosome(std::move(c), width, clen, std::move(nm), first);
      if (times) {  // (the walks of several chromosomes run side by side: each line is written whole)
        char line[160];
        const int k = snprintf(line, sizeof(line), "walk %u %.3f\n", clen, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        fwrite(line, 1, (size_t)k, times);
      }
      return o;
    }, std::move(cov), std::string(name)), close_tail});
    return K4_OK;
  }
  // the texts copied side by side into the one block the caller gets (gigabytes at low coverage)
  int finish(k4_index* ix, const char* header, K4HandOut& hand, char** block, uint64_t* bytes) {
    const size_t hn = header ? strlen(header) : 0;
    std::vector<WigOut> parts;
    parts.reserve(jobs.size());
    std::vector<size_t> at;
    size_t total = hn;
    for (Job& j : jobs) {
      parts.push_back(j.f.get());
      if (!j.close_tail) parts.back().tail.clear();
      at.push_back(total);
      total += parts.back().body.size() + parts.back().tail.size();
    }
    jobs.clear();
    K4_TRY(hand.block(ix, block, bytes, total));
    char* wo = *block;
    if (hn) memcpy(wo, header, hn);
    std::vector<std::future<void>> cp;
    for (size_t k = 0; k < parts.size(); k++)
      cp.push_back(std::async(std::launch::async, [&, k] {
        memcpy(wo + at[k], parts[k].body.data(), parts[k].body.size());
        memcpy(wo + at[k] + parts[k].body.size(), parts[k].tail.data(), parts[k].tail.size());
      }));
    for (std::future<void>& f : cp) f.get();
    return K4_OK;
  }
};

}  // namespace
