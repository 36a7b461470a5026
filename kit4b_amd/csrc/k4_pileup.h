// kit4b_amd/csrc/k4_pileup.h -- what the two readers of CKAligner::ProcessSNPs' per-locus base counts share: SNP calling
// (k4_snp.hip) and the packed base alleles of genpba (k4_pba.hip).  The pile-up of a chromosome's accepted alignments into seven
// count arrays, the pass that tells which sequences have any, and the walk that turns a chromosome's coverage into WIG spans.
// Everything sits in the including file's anonymous namespace: each of the two translation units compiles its own kernels.
#pragma once
#include <stdint.h>
#include <string.h>
#include <memory>
#include <string>
#include <hip/hip_runtime.h>
#include "k4_device.h"

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

}  // namespace
