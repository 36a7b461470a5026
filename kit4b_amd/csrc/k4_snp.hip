// kit4b_amd/csrc/k4_snp.hip -- kalign's SNP calling (main CSV) over device-resident alignments.
//
//   CKAligner::ProcessSNPs  ngskit4b/KAligner.cpp:8168-8590   per-locus base counts over the accepted alignments of a chromosome
//   CKAligner::OutputSNPs   ngskit4b/KAligner.cpp:7098-7760   background rate in a 51-base window, binomial p-value, Benjamini-
//                                                             Hochberg cut, one "SNP_ID",... CSV line per call
//   CStats::Binomial / ProbKeqlk / Calc_nCk   libkit4b/Stats.cpp:489-564
//
// Device: the pile-up (one wave per alignment, lanes over its bases, atomic adds into seven per-locus arrays of the chromosome),
// two prefix sums and one kernel that evaluates the window sums and the integer / proportion tests at every locus and appends the
// few loci that pass.  Host (this file, plain C++): error rates, p-values, ranks and text for those loci -- a few hundred per
// chromosome -- with the reference's own floating-point operations in its order (long double n-choose-k included).
// The files kalign writes beside it: the coverage WIG (host threads, one per chromosome) and the DiSNP / TriSNP haplotype files
// (:7767-8101; one thread per alignment finds the called loci it covers and counts its base combination for every run of two /
// three of them).  The pile-up, the walk over the sequences with alignments, the WIG queue and the hand-out of the texts live in
// k4_pileup.h: genpba's packed base alleles (k4_pba.hip) start from the same counts.  A run is one SnpRun and named steps over it
// (snp_sequence has their order); every entry point fills a SnpOpts and comes through snp_files.  Not built: the BED form.  Equal p-values keep locus order in the ranking (the
// reference's multi-threaded quicksort leaves them in no defined order).
// With the options of k4_snp_run2_dev two more files come out of the same counts:
//   SNP centroids (kalign -7; :7380-7398, :8104-8133, :8626-8660): how often each of the 4^7 reference 7-mers lies around a locus
//   with enough coverage (NumInsts: one streaming kernel per chromosome, k4k_snp_centroid_insts, a histogram in LDS per workgroup)
//   and around a called SNP (NumSNPs and the base counts: on the host, from the 7-mer index the candidate kernel leaves in Cand.cent).
//   Marker sequences (kalign -K; :7494-7560): for every candidate locus that passed the noise test, the MarkerLen consensus bases
//   around it (k4k_snp_markers, one wave per candidate, the per-locus rule in k4_marker_classify.h); a candidate without a marker
//   is dropped BEFORE the p-values and the Benjamini-Hochberg cut, so every file of the run changes with -K.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "k4_device.h"
#include "k4_marker_classify.h"
#include "k4_pileup.h"
#include "k4_stage.h"

namespace {

struct Cand { uint32_t loci, n_ref, n_nonref, by_base[5], loc_mm, loc_m, ref_base, cent; };  // 48 bytes

#define K4_CENT_FLANK 3u                // cSNPCentfFlankLen
#define K4_CENT_BINS 16384u             // 4^7: cSNPCentroidEls
#define K4_CENT_NONE 0xffffffffu        // the locus has no 7-mer: too close to an end, or a non-ACGT symbol in the window

// the reference 7-mer around locus l as the centroid table's index (first base in the highest two bits, :7385-7394)
K4_DEV uint32_t snp_centroid_index(const SnpArgs& a, uint32_t l) {
  if (l < K4_CENT_FLANK || (uint64_t)l + K4_CENT_FLANK >= a.clen) return K4_CENT_NONE;
  uint32_t idx = 0;
  for (uint32_t k = 0; k < 2 * K4_CENT_FLANK + 1; k++) {
    const uint32_t b = k4d_ref_base(a.ix, a.cs + l - K4_CENT_FLANK + k) & 7u;
    if (b > 3) return K4_CENT_NONE;
    idx = (idx << 2) | b;
  }
  return idx;
}

// OutputSNPs' per-locus tests that need no error rate (:7375-7438): coverage, non-reference count and proportion; the window
// [l - 25, l + 26) clamped into the chromosome as the reference's sliding sums have it
__global__ void __launch_bounds__(256) k4k_snp_candidates(SnpArgs a, const uint64_t* __restrict__ p_ref, const uint64_t* __restrict__ p_non,
                                                          int min_snp_reads, double nonref_frac, Cand* __restrict__ out, uint32_t cap,
                                                          uint32_t* __restrict__ n_out, int want_cent) {
  const uint32_t l = blockIdx.x * 256u + threadIdx.x;
  if (l >= a.clen) return;
  const size_t S = K4_SNP_STRIDE(a);
  const uint32_t n_ref = a.cnt[l], n_non = a.cnt[S + l];
  const int tot = (int)(n_ref + n_non);
  if (tot < min_snp_reads || n_non < 1) return;
  if ((double)n_non / tot < nonref_frac) return;
  const uint32_t flank = 25, win = 51;
  uint32_t lo = 0, hi = min(win, a.clen);
  if (a.clen > win) {  // slid once for every locus in (flank, clen - flank): it stays where the first / last of them left it
    lo = l <= flank ? 0u : (l + flank < a.clen ? l - flank : a.clen - win);
    hi = lo + win;
  }
  const uint32_t loc_mm = (uint32_t)(p_non[hi] - p_non[lo]), loc_m = (uint32_t)(p_ref[hi] - p_ref[lo]);
  const uint32_t slot = atomicAdd(n_out, 1u);
  if (slot >= cap) return;
  Cand c;
  c.loci = l; c.n_ref = n_ref; c.n_nonref = n_non;
  for (int b = 0; b < 5; b++) c.by_base[b] = a.cnt[(2 + b) * S + l];
  c.loc_mm = loc_mm; c.loc_m = loc_m;
  c.ref_base = k4d_ref_base(a.ix, a.cs + l);  // pSNP->RefBase: the target symbol (a covered locus: the reference has set it)
  c.cent = want_cent ? snp_centroid_index(a, l) : 0u;  // (a few hundred candidates per chromosome: seven symbol look-ups each are nothing)
  out[slot] = c;
}

// SNP centroids, NumInsts (:7377-7398): every locus of the chromosome with at least MinSNPreads bases counts for the reference 7-mer
// around it.  One streaming pass over the two coverage arrays: a thread takes four consecutive loci (one 16-byte load per array, as
// k4k_pba_classify), and only where one of them is covered deeply enough does it walk the ten reference symbols its four windows
// span -- rolled through a 14-bit index, two bits per locus, with a 7-bit mask of the non-ACGT symbols beside it (K4Tb: one packed
// word, one look-up of a flagged block for the whole walk).  A symbol outside the chromosome enters as non-ACGT, which is the
// reference's bounds test (Loci >= 3 && Loci < ChromLen - 3).
// The histogram is private to the workgroup: 16384 uint32 bins = 64 KiB of LDS, so two workgroups of 512 threads share a CU's
// 160 KiB (16 waves per CU, enough for a pass that waits on memory); a workgroup strides over tiles of 2048 loci and adds its
// non-zero bins to the run's 64-bit table at the end (a 32-bit bin holds a workgroup's share: far fewer than 2^32 loci).
#define K4_CENT_LPT 4u
#define K4_CENT_THREADS 512u
__global__ void __launch_bounds__(K4_CENT_THREADS) k4k_snp_centroid_insts(SnpArgs a, int min_snp_reads, unsigned long long* __restrict__ table) {
  __shared__ uint32_t bins[K4_CENT_BINS];
  for (uint32_t k = threadIdx.x; k < K4_CENT_BINS; k += K4_CENT_THREADS) bins[k] = 0;
  __syncthreads();
  const size_t S = K4_SNP_STRIDE(a);
  const uint64_t tile = (uint64_t)K4_CENT_THREADS * K4_CENT_LPT;
  K4Tb tb;
  tb.init(a.ix);
  for (uint64_t t0 = (uint64_t)blockIdx.x * tile; t0 < a.clen; t0 += (uint64_t)gridDim.x * tile) {
    const uint64_t l0 = t0 + (uint64_t)threadIdx.x * K4_CENT_LPT;
    if (l0 >= a.clen) continue;
    uint32_t nr[K4_CENT_LPT], nn[K4_CENT_LPT];
    k4d_load_words<K4_CENT_LPT>(a.cnt + l0, nr);      // (the arrays carry 16 zeroed words behind the chromosome)
    k4d_load_words<K4_CENT_LPT>(a.cnt + S + l0, nn);
    bool any = false;
#pragma unroll
    for (uint32_t j = 0; j < K4_CENT_LPT; j++) any |= (int)(nr[j] + nn[j]) >= min_snp_reads;
    if (!any) continue;
    uint32_t idx = 0, bad = 0;
#pragma unroll
    for (uint32_t k = 0; k < K4_CENT_LPT + 2 * K4_CENT_FLANK; k++) {  // symbols l0 - 3 .. l0 + 6; after symbol l + 3 the window of l is whole
      const int64_t l = (int64_t)l0 + k - K4_CENT_FLANK;
      const uint32_t b = l >= 0 && l < (int64_t)a.clen ? tb.get((int64_t)a.cs + l) : 4u;
      idx = ((idx << 2) | (b & 3u)) & (K4_CENT_BINS - 1u);
      bad = ((bad << 1) | (b > 3 ? 1u : 0u)) & 0x7fu;
      if (k >= 2 * K4_CENT_FLANK) {
        const uint32_t j = k - 2 * K4_CENT_FLANK;
        if (!bad && (int)(nr[j] + nn[j]) >= min_snp_reads) atomicAdd(&bins[idx], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < K4_CENT_BINS; k += K4_CENT_THREADS)
    if (bins[k]) atomicAdd(&table[k], (unsigned long long)bins[k]);
}

// Marker sequences (:7494-7545): one wave per candidate locus.  The tests on the candidate itself (inside the chromosome with its
// flanks, its own non-reference proportion at least 0.5) first; then the lanes stride over the MarkerLen loci, apply the per-locus
// rule and write the base; the wave gathers whether any locus rejected and how many are polymorphic; last the centre's base against
// the reference base there.  Per candidate: hdr[2 w] = 1 accepted / 0 rejected, hdr[2 w + 1] = NumPolymorphicSites, seq[w * len ..].
__global__ void __launch_bounds__(256) k4k_snp_markers(SnpArgs a, const uint32_t* __restrict__ loci, uint32_t n, int marker_len, int min_snp_reads,
                                                       double poly_thres, uint32_t* __restrict__ hdr, uint8_t* __restrict__ seq) {
  const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
  if (w >= n) return;  // (whole waves leave: the shuffles below see all their lanes)
  const size_t S = K4_SNP_STRIDE(a);
  const uint32_t m5 = (uint32_t)marker_len / 2u, m3 = (uint32_t)marker_len - 1u - m5;  // m_Marker5Len, m_Marker3Len (:260-261)
  const uint32_t l = loci[w];
  bool ok = l < a.clen && l >= m5 && (uint64_t)l + m3 < a.clen;
  if (ok) {
    const uint32_t n_ref = a.cnt[l], n_non = a.cnt[S + l];
    const int tot = (int)(n_non + n_ref);
    ok = tot > 0 && !((double)n_non / tot < 0.5);
  }
  uint32_t poly = 0, centre = 0;
  bool rej = false;
  if (ok) {
    for (uint32_t q = lane; q < (uint32_t)marker_len; q += 64u) {
      const uint32_t ml = l - m5 + q;
      const uint32_t by_base[5] = {a.cnt[2 * S + ml], a.cnt[3 * S + ml], a.cnt[4 * S + ml], a.cnt[5 * S + ml], a.cnt[6 * S + ml]};
      int p = 0;
      const int b = k4_marker_base(a.cnt[ml], a.cnt[S + ml], by_base, k4d_ref_base(a.ix, a.cs + ml) & 7u, min_snp_reads, poly_thres, &p);
      if (b < 0) { rej = true; continue; }
      poly += (uint32_t)p;
      seq[(size_t)w * (uint32_t)marker_len + q] = (uint8_t)"ACGTN"[b];
      if (q == m5) centre = (uint32_t)b;
    }
  }
  for (int d = 32; d > 0; d >>= 1) poly += __shfl_down(poly, d, 64);
  const bool any_rej = __ballot(rej) != 0ull;
  centre = __shfl(centre, (int)(m5 & 63u), 64);
  if (lane == 0) {
    uint32_t ref = k4d_ref_base(a.ix, a.cs + (l < a.clen ? l : 0u)) & 7u;
    if (ref > 4) ref = 4;
    hdr[2 * w] = ok && !any_rej && centre != ref ? 1u : 0u;  // (:7543: the centre must not call the reference base)
    hdr[2 * w + 1] = poly;
  }
}

// coverage per locus (TotBases) for the WIG: ref + nonref.  First its maximum, then the array in the narrowest of 1 / 2 / 4 bytes
// per locus that holds it (whole-genome coverage fits a byte: a quarter of the bytes to bring down and to walk through)
__global__ void __launch_bounds__(256) k4k_snp_coverage_max(const uint32_t* __restrict__ ref, const uint32_t* __restrict__ non, uint32_t n,
                                                            uint32_t* __restrict__ mx) {
  uint32_t m = 0;
  for (uint32_t l = blockIdx.x * 256u + threadIdx.x; l < n; l += gridDim.x * 256u) m = max(m, ref[l] + non[l]);
  for (int d = 32; d > 0; d >>= 1) m = max(m, (uint32_t)__shfl_down(m, d, 64));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(mx, m);
}
template <typename T>
__global__ void __launch_bounds__(256) k4k_snp_coverage(const uint32_t* __restrict__ ref, const uint32_t* __restrict__ non, uint32_t n,
                                                        T* __restrict__ cov) {
  const uint32_t l = blockIdx.x * 256u + threadIdx.x;
  if (l < n) cov[l] = (T)(ref[l] + non[l]);
}

// DiSNPs / TriSNPs (OutputSNPs :7767-8101 with IterateReadsOverlapping :10475-10546 and AdjAlignSNPBase :1581-1632): for two / three
// called loci following each other closely, the alignments that cover all of them and the bases they show there.  The reference
// walks the sorted alignments once per locus pair; here every alignment looks up the called loci inside its span (they are sorted)
// and adds itself to the pair ending at each of them (slot from the host: -1 = loci too far apart) -- 16 combination counters + the
// antisense count per pair, 64 + 1 per triple.
struct HapArgs {
  const uint32_t* loci;     // called SNP loci of the chromosome, ascending
  const int32_t* di_slot;   // per locus k: slot of the pair (k-1, k), or -1
  const int32_t* tri_slot;  // per locus k: slot of the triple (k-2, k-1, k), or -1
  uint32_t n_loci;
  uint32_t* di;             // [n_di][17]
  uint32_t* tri;            // [n_tri][65]
};
__global__ void __launch_bounds__(256) k4k_snp_haplotypes(SnpArgs a, HapArgs hp) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.rs.n_reads; i += (int64_t)gridDim.x * 256) {
    if (a.rs.nar(i) != K4_NAR_ACCEPTED) continue;
    const k4_hit h = a.rs.hit(i);
    if (h.chrom_id != a.chrom_id || (h.ext & (K4_EXT_INDEL | K4_EXT_SPLICE))) continue;
    const uint32_t match_len = k4d_adj_len(h);
    const uint32_t start = k4d_adj_start(h);  // AdjStartLoci .. AdjEndLoci
    if (match_len == 0 || (uint64_t)start + match_len > a.clen) continue;
    const uint32_t end = start + match_len - 1;
    uint32_t lo = 0, hi = hp.n_loci;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (hp.loci[mid] < start) lo = mid + 1; else hi = mid;
    }
    const uint8_t* bases = a.rs.reads + a.rs.offs[i];
    const bool anti = h.strand != '+';
    uint32_t b1 = 7, b2 = 7;  // the read's bases at the two loci before this one
    for (uint32_t k = lo; k < hp.n_loci; k++) {
      const uint32_t l = hp.loci[k];
      if (l > end) break;
      uint32_t b = anti ? (bases[h.match_loci + (uint32_t)h.match_len - l - 1] & 7u) : (bases[l - h.match_loci] & 7u);
      if (anti && b <= 3) b = 3 - b;
      if (k >= lo + 1 && b <= 3 && b1 <= 3) {
        const int32_t sd = hp.di_slot[k];
        if (sd >= 0) {
          atomicAdd(&hp.di[(size_t)sd * 17 + ((b1 << 2) | b)], 1u);
          if (anti) atomicAdd(&hp.di[(size_t)sd * 17 + 16], 1u);
        }
        if (k >= lo + 2 && b2 <= 3) {
          const int32_t st = hp.tri_slot[k];
          if (st >= 0) {
            atomicAdd(&hp.tri[(size_t)st * 65 + ((b2 << 4) | (b1 << 2) | b)], 1u);
            if (anti) atomicAdd(&hp.tri[(size_t)st * 65 + 64], 1u);
          }
        }
      }
      b2 = b1; b1 = b;
    }
  }
}

// one line of the .disnp.csv / .trisnp.csv file (:7836-7916, :7997-8089) from a slot's counters; false = not reported (too few
// reads or haplotypes).  A combination counts as a haplotype from max(5, a tenth of the covering reads) reads on.
static bool hap_line(std::string& out, const char* type, int id, const std::string& species, const char* chrom, const uint32_t* loci,
                     const uint32_t* ref, int n, const uint32_t* c, int min_snp_reads) {
  const int nc = n == 2 ? 16 : 64;
  int by_base[3][4] = {{0}}, depth = 0, cnts[64];
  for (int q = 0; q < nc; q++) {
    cnts[q] = (int)c[q];
    depth += cnts[q];
    for (int k = 0; k < n; k++) by_base[k][(q >> (2 * (n - 1 - k))) & 3] += cnts[q];
  }
  if (depth < min_snp_reads) return false;
  const int thres = std::max(5, (depth + 5) / 10);
  int n_hap = 0;
  for (int q = 0; q < nc; q++) { if (cnts[q] >= thres) n_hap++; else cnts[q] = 0; }
  if (n_hap < n) return false;
  char line[1200];
  int m = snprintf(line, sizeof(line), "%d,\"%s\",\"%s\",\"%s\",", id, type, species.c_str(), chrom);
  for (int k = 0; k < n; k++)
    m += snprintf(line + m, sizeof(line) - m, "%d,\"%c\",%d,%d,%d,%d,0,", (int)loci[k], "acgtn"[ref[k] > 4 ? 4 : ref[k]], by_base[k][0], by_base[k][1],
                  by_base[k][2], by_base[k][3]);
  m += snprintf(line + m, sizeof(line) - m, "%d,%d,%d", depth, (int)c[nc], n_hap);
  for (int q = 0; q < nc; q++) m += snprintf(line + m, sizeof(line) - m, ",%d", cnts[q]);
  line[m++] = '\n';
  out.append(line, (size_t)m);
  return true;
}
static std::string hap_header(int n) {  // :8252-8330
  std::string s = n == 2 ? "\"DiSNPs_ID\"" : "\"TriSNPs_ID\"";
  s += ",\"ElType\",\"Species\",\"Chrom\"";
  for (int k = 1; k <= n; k++) {
    const std::string p = "\"SNP" + std::to_string(k);
    s += "," + p + "Loci\"," + p + "RefBase\"," + p + "BaseAcnt\"," + p + "BaseCcnt\"," + p + "BaseGcnt\"," + p + "BaseTcnt\"," + p + "BaseNcnt\"";
  }
  s += ",\"Depth\",\"Antisense\",\"Haplotypes\"";
  for (int q = 0; q < (n == 2 ? 16 : 64); q++) {
    s += ",\"";
    for (int j = n - 1; j >= 0; j--) s += "acgt"[(q >> (2 * j)) & 3];
    s += "\"";
  }
  return s + "\n";
}

// ---- CStats (libkit4b/Stats.cpp:489-564), operation for operation ------------------------------------------------------------
double calc_nck(uint32_t n, uint32_t k) {
  if (k > n) return 0.0;
  if (k > n / 2) k = n - k;
  long double accum = 1;
  for (uint32_t i = 1; i <= k; i++) accum = accum * (n - k + i) / i;
  return (double)accum;
}
double prob_k_eql_k(uint32_t n, uint32_t k, double p) {
  if (p < 0 || p > 1) return -1;
  const double nck = calc_nck(n, k);
  const double p2 = pow(p, (int32_t)k);
  const double q2 = pow(1 - p, (int32_t)(n - k));
  return nck * p2 * q2;
}
double binomial(int n, int k, double p) {
  if (k > n) return 0.0;
  if (n > 5000) { k = (int)((1000.0 / n) * k); n = 5000; }
  double sum = 0;
  for (int i = 0; i <= k; i++) {
    sum += prob_k_eql_k((uint32_t)n, (uint32_t)i, p);
    if (sum >= 1.0) break;
  }
  return std::min(sum, 1.0);
}

struct LociPV {
  uint32_t loci, rank, num_reads, num_subs, local_reads, local_subs, ref_base;
  uint32_t by_base[5];
  double pvalue, bkgnd;
  uint32_t cent, marker_id, n_poly;
};
struct Centroid { uint64_t n_insts, n_snps, ref_cnt, by_base[5]; };
const uint32_t kMarkerChunk = 4096;  // candidates per launch of k4k_snp_markers: one wave each fills the device; the output stays below 2.1 MB
const uint32_t kCandCap = 1u << 22;  // candidate loci per chromosome kept on the device (more: the call fails loudly)

// what an entry point asks of a run: kalign's options and which files it wants beside the SNP file
struct SnpOpts {
  int vcf;
  int32_t min_snp_reads;
  double qvalue, nonref_pcnt;
  bool want_wig, want_hap;
  int marker_len = 0;  // k4_snp_run2_dev: 0 = no markers
  double poly_thres = 0.0;
  bool want_centroids = false;
};

// ---- the host-only steps: plain functions of their inputs ------------------------------------------------------------------------
static std::string snp_header(int vcf, const std::string& dataset) {
  if (vcf)
    return "##fileformat=VCFv4.1\n##source=k4align1.0\n##reference=" + dataset +
           "\n##INFO=<ID=AF,Number=A,Type=Float,Description=\"Allele Frequency\">\n##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Read Depth\">\n"
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
  return "\"SNP_ID\",\"ElType\",\"Species\",\"Chrom\",\"StartLoci\",\"EndLoci\",\"Len\",\"Strand\",\"Rank\",\"PValue\",\"Bases\",\"Mismatches\",\"RefBase\","
         "\"MMBaseA\",\"MMBaseC\",\"MMBaseG\",\"MMBaseT\",\"MMBaseN\",\"BackgroundSubRate\",\"TotWinBases\",\"TotWinMismatches\",\"MarkerID\",\"NumPolymorphicSites\"\n";
}
// OutputSNPs' background rate and noise test (:7320, :7425-7450) over a sequence's candidates; tot: the pile-up's totals
static void snp_noise_gate(const std::vector<Cand>& hc, const unsigned long long* tot, std::vector<LociPV>* pv) {
  double global_rate = (double)tot[1] / (double)(1 + tot[0] + tot[1]);
  global_rate = std::max(0.005, global_rate);  // cMinSeqErrRate
  pv->clear();
  for (const Cand& c : hc) {
    const uint32_t ltmm = c.n_nonref <= c.loc_mm ? c.loc_mm - c.n_nonref : 0;
    const uint32_t ltm = c.n_ref < c.loc_m ? c.loc_m - c.n_ref : 0;
    double local_rate;
    if ((ltmm + ltm) == 0) local_rate = global_rate;
    else {
      local_rate = (double)ltmm / (double)(ltmm + ltm);
      if (local_rate < global_rate) local_rate = global_rate;
    }
    if (local_rate > 0.20) continue;  // cMaxBkgdNoiseThres
    LociPV p;
    const int tot_bases = (int)(c.n_ref + c.n_nonref);
    p.pvalue = 0.0; p.cent = c.cent; p.marker_id = 0; p.n_poly = 0;
    p.loci = c.loci; p.rank = 0; p.bkgnd = local_rate; p.local_reads = ltmm + ltm; p.local_subs = ltmm;
    p.num_reads = (uint32_t)tot_bases; p.num_subs = c.n_nonref;
    for (int b = 0; b < 5; b++) p.by_base[b] = c.by_base[b];
    p.ref_base = c.ref_base > 4 ? 4 : c.ref_base;
    pv->push_back(p);
  }
}
// ranks by p-value (equal ones keep locus order: a stable sort), Benjamini-Hochberg at qvalue (:7567-7640); leaves the accepted
// loci, ranked, in locus order
static void snp_bh_cut(std::vector<LociPV>* pv, double qvalue) {
  std::stable_sort(pv->begin(), pv->end(), [](const LociPV& x, const LociPV& y) { return x.pvalue < y.pvalue; });
  size_t n_acc = 0;
  for (size_t k = 0; k < pv->size(); k++) {
    const double adj = ((k + 1) / (double)pv->size()) * qvalue;
    if ((*pv)[k].pvalue >= adj) break;
    (*pv)[k].rank = (uint32_t)(k + 1);
    n_acc++;
  }
  pv->resize(n_acc);
  std::sort(pv->begin(), pv->end(), [](const LociPV& x, const LociPV& y) { return x.loci < y.loci; });
}
// a VCF record (:7650-7696): alternative alleles with at least a tenth of the strongest one's count, their frequencies, phred of the
// p-value.  alts / freq are the run's: the reference never clears its two strings, so a SNP whose mismatches are all N prints what
// the SNP before it left there
static void snp_vcf_line(std::string* text, const char* chrom, const LociPV& p, uint64_t id, char* alts, char* freq) {
  uint32_t thres = 0;
  for (uint32_t b = 0; b < 4; b++)
    if (b != p.ref_base && p.by_base[b] > thres) thres = p.by_base[b];
  thres = std::max((thres + 5) / 10, 1u);
  int ao = 0, fo = 0;
  for (uint32_t b = 0; b < 4; b++) {
    if (b == p.ref_base || p.by_base[b] < thres) continue;
    if (ao > 0) { alts[ao++] = ','; freq[fo++] = ','; }
    alts[ao++] = "ACGT"[b]; alts[ao] = 0;
    fo += sprintf(&freq[fo], "%1.4f", (double)p.by_base[b] / p.num_reads);
  }
  const int phred = p.pvalue < 0.0000000001 ? 100 : (int)(0.5 + (10.0 * log10(1.0 / p.pvalue)));
  char line[512];
  const int n = snprintf(line, sizeof(line), "%s\t%u\tSNP%d\t%c\t%s\t%d\tPASS\tAF=%s;DP=%d\n", chrom, p.loci + 1, (int)id, "ACGTN"[p.ref_base], alts, phred, freq,
                         (int)p.num_reads);
  text->append(line, (size_t)n);
}
// a line of the main CSV (:7698-7760); n_acc: the sequence's called loci, which the score is relative to
static void snp_csv_line(std::string* text, const std::string& dataset, const char* chrom, LociPV p, uint64_t id, size_t n_acc) {
  int rel = (int)(999 - ((999 * (int64_t)p.rank) / (int64_t)n_acc));
  if (rel < 1) rel = 1;
  p.by_base[p.ref_base] = p.num_reads - p.num_subs;  // :7698 (on this path only, and behind the centroid tally)
  char line[512];
  const int n = snprintf(line, sizeof(line), "%d,\"SNP\",\"%s\",\"%s\",%d,%d,1,\"+\",%d,%f,%d,%d,\"%c\",%d,%d,%d,%d,%d,%f,%d,%d,%d,%d\n", (int)id, dataset.c_str(),
                         chrom, (int)p.loci, (int)p.loci, rel, p.pvalue, (int)p.num_reads, (int)p.num_subs, "ACGTN"[p.ref_base], (int)p.by_base[0],
                         (int)p.by_base[1], (int)p.by_base[2], (int)p.by_base[3], (int)p.by_base[4], p.bkgnd, (int)p.local_reads, (int)p.local_subs,
                         (int)p.marker_id, (int)p.n_poly);
  text->append(line, (size_t)n);
}
// the centroid file (:8626-8660): every 7-mer, whether seen or not
static std::string snp_centroid_text(const std::vector<unsigned long long>& insts, const std::vector<Centroid>& rows) {
  std::string ct = "\"CentroidID\",\"Seq\",\"NumInsts\",\"NumSNPs\",\"RefBase\",\"RefBaseCnt\",\"BaseA\",\"BaseC\",\"BaseG\",\"BaseT\",\"BaseN\"\n";
  char line[256];
  for (uint32_t id = 0; id < K4_CENT_BINS; id++) {
    char sq[8];
    for (int k = 0; k < 7; k++) sq[k] = "ACGT"[(id >> (2 * (6 - k))) & 3u];
    sq[7] = 0;
    const Centroid& r = rows[id];
    const int n = snprintf(line, sizeof(line), "%d,\"%s\",%d,%d,\"%c\",%d,%d,%d,%d,%d,%d\n", (int)id + 1, sq, (int)insts[id], (int)r.n_snps, sq[3], (int)r.ref_cnt,
                           (int)r.by_base[0], (int)r.by_base[1], (int)r.by_base[2], (int)r.by_base[3], (int)r.by_base[4]);
    ct.append(line, (size_t)n);
  }
  return ct;
}

// a run: the walk over the sequences, the device buffers of SNP calling alone, what the sequences leave behind, and the steps
// (snp_sequence has their order)
struct SnpRun {
  k4_index* ix = nullptr;
  hipStream_t st = nullptr;
  SnpOpts o;
  PileupWalk w;
  SnpArgs& a = w.a;                    // of the sequence the walk handed out last
  WigQueue wig;
  K4DevBuf pref, pnon, cands, ncand, covb, covmax;
  K4DevBuf cent_tab, mk_loci, mk_out;  // the run's centroid instance counts; a chunk of candidate loci and their markers
  K4Scratch<K4DevBuf> tmp;             // of the prefix sums: sized for the longest sequence, once
  std::vector<Cand> hc;                // the sequence's candidates, in locus order
  std::vector<LociPV> pv;              // ... those still in the running
  std::string text, di, tri, markers, centroids;
  std::vector<Centroid> cent_rows;
  uint64_t n_markers = 0, tot_snps = 0;  // m_MarkerID and the SNP ids: both run across sequences
  char alts[100] = "", freq[100] = ""; // VCF: ALT and AF of the last SNP that had any (see snp_vcf_line)

  int snp_open(k4_index* ix_, const K4Records& rec, const SnpOpts& o_, void* stream) {
    ix = ix_;
    o = o_;
    if (rec.n_units < 0 || o.min_snp_reads < 1 || o.qvalue < 0.0 || o.nonref_pcnt < 0.0) return k4_fail(ix, K4_ERR_PARAMS, "SNP parameters out of range");
    if (o.marker_len != 0 && (o.marker_len < 25 || o.marker_len > 500 || !(o.poly_thres >= 0.0 && o.poly_thres <= 0.5)))  // cMinMarkerLen .. cMaxMarkerLen
      return k4_fail(ix, K4_ERR_PARAMS, "marker length must be 0 or 25..500 and the marker polymorphism threshold 0.0..0.5");
    K4_TRY(w.open(ix, rec, stream));
    st = w.st;
    text = snp_header(o.vcf, ix->dataset);
    di = hap_header(2);
    tri = hap_header(3);
    const size_t S = w.S;
    K4_HIP(ix, pref.alloc((S + 1) * 8));
    K4_HIP(ix, pnon.alloc((S + 1) * 8));
    K4_HIP(ix, cands.alloc((size_t)kCandCap * sizeof(Cand)));
    K4_HIP(ix, ncand.alloc(4));
    if (o.want_centroids) {  // :8319-8332
      cent_rows.assign(K4_CENT_BINS, Centroid{0, 0, 0, {0, 0, 0, 0, 0}});
      K4_HIP(ix, cent_tab.alloc((size_t)K4_CENT_BINS * 8));
      K4_HIP(ix, hipMemsetAsync(cent_tab.p, 0, (size_t)K4_CENT_BINS * 8, st));
    }
    if (o.marker_len) {
      K4_HIP(ix, mk_loci.alloc((size_t)kMarkerChunk * 4));
      K4_HIP(ix, mk_out.alloc((size_t)kMarkerChunk * ((size_t)o.marker_len + 8)));
    }
    return k4s_exclusive_scan(ix, (const uint32_t*)nullptr, pref.as<uint64_t>(), (uint64_t)0, S + 1, rocprim::plus<uint64_t>(), st, &tmp, true);
  }
  // SNP centroids, NumInsts of every locus of this sequence (independent of SNP calling, :7380-7398)
  int snp_centroid_insts() {
    const uint64_t tiles = ((uint64_t)a.clen + K4_CENT_THREADS * K4_CENT_LPT - 1) / (K4_CENT_THREADS * K4_CENT_LPT);
    hipLaunchKernelGGL(k4k_snp_centroid_insts, dim3((unsigned)std::min<uint64_t>(tiles, 512)), dim3(K4_CENT_THREADS), 0, st, a, (int)o.min_snp_reads,
                       cent_tab.as<unsigned long long>());
    K4_HIP(ix, hipGetLastError());
    return K4_OK;
  }
  // the sequence's coverage in the narrowest form, into the WIG queue: loci counted from 0, the tail left open until a candidate turns up
  int snp_queue_wig(size_t* slot) {
    const uint32_t* non = a.cnt + K4_SNP_STRIDE(a);
    if (!covb.p) { K4_HIP(ix, covb.alloc(w.S * 4)); K4_HIP(ix, covmax.alloc(4)); }
    K4_HIP(ix, hipMemsetAsync(covmax.p, 0, 4, st));
    hipLaunchKernelGGL(k4k_snp_coverage_max, dim3(1024), dim3(256), 0, st, a.cnt, non, a.clen, covmax.as<uint32_t>());
    K4_HIP(ix, hipGetLastError());
    uint32_t mx = 0;
    K4_TRY(k4s_read_back(ix, &mx, covmax.p, st));
    const int width = mx < 256 ? 1 : mx < 65536 ? 2 : 4;
    const dim3 cg((a.clen + 255) / 256);
    if (width == 1) hipLaunchKernelGGL(k4k_snp_coverage<uint8_t>, cg, dim3(256), 0, st, a.cnt, non, a.clen, covb.as<uint8_t>());
    else if (width == 2) hipLaunchKernelGGL(k4k_snp_coverage<uint16_t>, cg, dim3(256), 0, st, a.cnt, non, a.clen, covb.as<uint16_t>());
    else hipLaunchKernelGGL(k4k_snp_coverage<uint32_t>, cg, dim3(256), 0, st, a.cnt, non, a.clen, covb.as<uint32_t>());
    K4_HIP(ix, hipGetLastError());
    return wig.add(ix, st, covb.p, width, a.clen, w.e->name, 0u, false, slot);
  }
  // the loci that pass the tests that need no error rate, in locus order: two prefix sums over [0, clen] (element l = sum of the loci
  // below l; the arrays are zero behind clen), the candidate kernel, its list brought down
  int snp_candidates() {
    K4_HIP(ix, hipMemsetAsync(ncand.p, 0, 4, st));
    K4_TRY(k4s_exclusive_scan(ix, a.cnt, pref.as<uint64_t>(), (uint64_t)0, (size_t)a.clen + 1, rocprim::plus<uint64_t>(), st, &tmp));
    K4_TRY(k4s_exclusive_scan(ix, a.cnt + K4_SNP_STRIDE(a), pnon.as<uint64_t>(), (uint64_t)0, (size_t)a.clen + 1, rocprim::plus<uint64_t>(), st, &tmp));
    hipLaunchKernelGGL(k4k_snp_candidates, dim3((a.clen + 255) / 256), dim3(256), 0, st, a, pref.as<uint64_t>(), pnon.as<uint64_t>(), (int)o.min_snp_reads,
                       o.nonref_pcnt / 100.0 /* m_SNPNonRefPcnt, KAligner.cpp:256 */, cands.as<Cand>(), kCandCap, ncand.as<uint32_t>(), o.want_centroids ? 1 : 0);
    K4_HIP(ix, hipGetLastError());
    uint32_t nc = 0;
    K4_TRY(k4s_read_back(ix, &nc, ncand.p, st));
    if (nc > kCandCap) return k4_fail(ix, K4_ERR_MEM, "more than %u candidate SNP loci on %s", kCandCap, w.e->name);
    hc.resize(nc);
    if (nc) K4_HIP(ix, hipMemcpyAsync(hc.data(), cands.p, (size_t)nc * sizeof(Cand), hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipStreamSynchronize(st));
    std::sort(hc.begin(), hc.end(), [](const Cand& x, const Cand& y) { return x.loci < y.loci; });
    return K4_OK;
  }
  // the marker gate (:7494-7560): in locus order, chunk by chunk; a candidate without a marker leaves pv here
  int snp_marker_gate() {
    const int marker_len = o.marker_len, m5 = marker_len / 2;
    const size_t row = (size_t)marker_len;
    std::vector<uint32_t> mk_l;
    std::vector<uint8_t> mk_h;
    size_t kept = 0;
    char head[600];
    for (size_t c0 = 0; c0 < pv.size(); c0 += kMarkerChunk) {
      const uint32_t nq = (uint32_t)std::min<size_t>(kMarkerChunk, pv.size() - c0);
      mk_l.resize(nq);
      for (uint32_t k = 0; k < nq; k++) mk_l[k] = pv[c0 + k].loci;
      uint32_t* d_hdr = mk_out.as<uint32_t>();
      uint8_t* d_seq = mk_out.as<uint8_t>() + (size_t)nq * 8;
      K4_HIP(ix, hipMemcpyAsync(mk_loci.p, mk_l.data(), (size_t)nq * 4, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k4k_snp_markers, dim3((nq + 3) / 4), dim3(256), 0, st, w.a, mk_loci.as<uint32_t>(), nq, marker_len, (int)o.min_snp_reads,
                         o.poly_thres, d_hdr, d_seq);
      K4_HIP(ix, hipGetLastError());
      mk_h.resize((size_t)nq * (row + 8));
      K4_HIP(ix, hipMemcpyAsync(mk_h.data(), mk_out.p, mk_h.size(), hipMemcpyDeviceToHost, st));
      K4_HIP(ix, hipStreamSynchronize(st));
      for (uint32_t k = 0; k < nq; k++) {
        uint32_t h2[2];
        memcpy(h2, &mk_h[(size_t)k * 8], 8);
        if (!h2[0]) continue;
        LociPV p = pv[c0 + k];
        const uint8_t* sq = &mk_h[(size_t)nq * 8 + (size_t)k * row];
        p.marker_id = (uint32_t)++n_markers;
        p.n_poly = h2[1];
        // >MarkerNNN Chrom StartLoci|MarkerLen|SNPLoci|Marker5Len|SNPbase|RefBase|NumPolymorphicSites (:7552)
        const int hn = snprintf(head, sizeof(head), ">Marker%d %s %d|%d|%d|%d|%c|%c|%d\n", (int)p.marker_id, w.e->name, (int)p.loci - m5, marker_len, (int)p.loci,
                                m5, (char)sq[m5], "ACGTN"[p.ref_base], (int)p.n_poly);
        markers.append(head, (size_t)std::min<int>(hn, (int)sizeof(head) - 1));
        markers.append((const char*)sq, row);
        markers += '\n';
        pv[kept++] = p;  // (kept <= c0 + k: nothing is overwritten before it is read)
      }
    }
    pv.resize(kept);
    return K4_OK;
  }
  // DiSNPs / TriSNPs of this sequence (:7767-8101) over its called loci pv: the slots on the host, the counters from the device
  int snp_haplotypes() {
    const size_t n_acc = pv.size();
    const char* chrom = w.e->name;
    const int mean_len = (int)(uint32_t)((w.t[3] + w.t[2] - 1) / w.t[2]);
    const int max_sep = std::min(300, mean_len);  // m_MaxDiSNPSep = min(cDfltMaxDiSNPSep, MeanReadLen), :7346
    std::vector<uint32_t> loci(n_acc);
    std::vector<int32_t> slot(2 * n_acc, -1);  // [0, n_acc): pair ending at k, [n_acc, 2 n_acc): triple ending at k
    uint32_t n_di = 0, n_tri = 0;
    for (size_t k = 0; k < n_acc; k++) {
      loci[k] = pv[k].loci;
      const int cur = (int)pv[k].loci;
      if (k >= 1 && cur > 0 && cur - (int)pv[k - 1].loci <= max_sep) slot[k] = (int32_t)n_di++;
      if (k >= 2 && pv[k - 1].loci > 0 && cur > 0 && cur - (int)pv[k - 2].loci <= max_sep) slot[n_acc + k] = (int32_t)n_tri++;
    }
    if (!n_di) return K4_OK;  // (a triple holds two pairs: no pair, no triple)
    K4DevBuf dl, ds, dd, dt;
    K4_HIP(ix, dl.alloc(n_acc * 4));
    K4_HIP(ix, ds.alloc(2 * n_acc * 4));
    K4_HIP(ix, dd.alloc((size_t)n_di * 17 * 4));
    K4_HIP(ix, dt.alloc((size_t)n_tri * 65 * 4));
    K4_HIP(ix, hipMemcpyAsync(dl.p, loci.data(), n_acc * 4, hipMemcpyHostToDevice, st));
    K4_HIP(ix, hipMemcpyAsync(ds.p, slot.data(), 2 * n_acc * 4, hipMemcpyHostToDevice, st));
    K4_HIP(ix, hipMemsetAsync(dd.p, 0, (size_t)n_di * 17 * 4, st));
    if (n_tri) K4_HIP(ix, hipMemsetAsync(dt.p, 0, (size_t)n_tri * 65 * 4, st));
    HapArgs hp;
    hp.loci = dl.as<uint32_t>(); hp.di_slot = ds.as<int32_t>(); hp.tri_slot = ds.as<int32_t>() + n_acc; hp.n_loci = (uint32_t)n_acc;
    hp.di = dd.as<uint32_t>(); hp.tri = dt.as<uint32_t>();
    const int64_t nb = std::min<int64_t>((w.a.rs.n_reads + 255) / 256, 8192);
    hipLaunchKernelGGL(k4k_snp_haplotypes, dim3((unsigned)nb), dim3(256), 0, st, w.a, hp);
    K4_HIP(ix, hipGetLastError());
    std::vector<uint32_t> hd((size_t)n_di * 17), ht((size_t)n_tri * 65);
    K4_HIP(ix, hipMemcpyAsync(hd.data(), dd.p, hd.size() * 4, hipMemcpyDeviceToHost, st));
    if (n_tri) K4_HIP(ix, hipMemcpyAsync(ht.data(), dt.p, ht.size() * 4, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipStreamSynchronize(st));
    int tot_di = 0, tot_tri = 0;  // (the ids restart with every chromosome, :7634-7635)
    for (size_t k = 1; k < n_acc; k++) {
      if (slot[k] >= 0) {
        const uint32_t l2[2] = {pv[k - 1].loci, pv[k].loci}, r2[2] = {pv[k - 1].ref_base, pv[k].ref_base};
        if (hap_line(di, "DiSNPs", tot_di + 1, ix->dataset, chrom, l2, r2, 2, &hd[(size_t)slot[k] * 17], o.min_snp_reads)) tot_di++;
      }
      if (k >= 2 && slot[n_acc + k] >= 0) {
        const uint32_t l3[3] = {pv[k - 2].loci, pv[k - 1].loci, pv[k].loci}, r3[3] = {pv[k - 2].ref_base, pv[k - 1].ref_base, pv[k].ref_base};
        if (hap_line(tri, "TriSNPs", tot_tri + 1, ix->dataset, chrom, l3, r3, 3, &ht[(size_t)slot[n_acc + k] * 65], o.min_snp_reads)) tot_tri++;
      }
    }
    return K4_OK;
  }
  // the sequence's called SNPs into the SNP file and the centroid tallies
  void snp_emit() {
    for (const LociPV& p : pv) {
      tot_snps++;
      if (o.want_centroids && p.cent != K4_CENT_NONE) {  // the called SNP's counts as piled, for the 7-mer around it (:8104-8133)
        Centroid& c = cent_rows[p.cent];
        c.n_snps++;
        c.ref_cnt += p.num_reads - p.num_subs;
        for (int b = 0; b < 5; b++) c.by_base[b] += p.by_base[b];
      }
      if (o.vcf) snp_vcf_line(&text, w.e->name, p, tot_snps, alts, freq);
      else snp_csv_line(&text, ix->dataset, w.e->name, p, tot_snps, pv.size());
    }
  }
  // OutputSNPs for the sequence the walk has just piled up (:7320-7640)
  int snp_sequence() {
    if (o.want_centroids) K4_TRY(snp_centroid_insts());
    size_t wig_slot = 0;
    if (o.want_wig) K4_TRY(snp_queue_wig(&wig_slot));  // (its walk runs on a thread of its own from here on)
    K4_TRY(snp_candidates());
    snp_noise_gate(hc, w.t, &pv);
    if (o.marker_len && !pv.empty()) K4_TRY(snp_marker_gate());  // (before the p-values: every file of the run changes with -K)
    for (LociPV& p : pv) p.pvalue = 1.0 - binomial((int)p.num_reads, (int)p.num_subs, p.bkgnd);
    // decided before the cut: a chromosome without a candidate never closes its last span, one whose candidates all fall to the cut does
    if (o.want_wig && !pv.empty()) wig.jobs[wig_slot].close_tail = true;
    if (pv.empty()) return K4_OK;
    snp_bh_cut(&pv, o.qvalue);
    if (o.want_hap && pv.size() >= 2) K4_TRY(snp_haplotypes());
    snp_emit();
    return K4_OK;
  }
  // the centroid instance counts down, the file's text
  int snp_centroid_file() {
    std::vector<unsigned long long> insts(K4_CENT_BINS);
    K4_HIP(ix, hipMemcpyAsync(insts.data(), cent_tab.p, (size_t)K4_CENT_BINS * 8, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipStreamSynchronize(st));
    centroids = snp_centroid_text(insts, cent_rows);
    return K4_OK;
  }
};

// a whole run into `out`: every member the options ask for, the others null.  Every entry point comes through here; on an error
// the guard leaves `out` zeroed and nothing handed out.
static int snp_files(k4_index* ix, const K4Records& rec, const SnpOpts& o, k4_snp_files2* out, void* stream) {
  K4HandOut hand(out);
  if (!ix) return K4_ERR_PARAMS;
  SnpRun r;
  K4_TRY(r.snp_open(ix, rec, o, stream));
  for (bool got = false;;) {  // the sorted reads: one chromosome after the other
    K4_TRY(r.w.next(&got));
    if (!got) break;
    K4_TRY(r.snp_sequence());
  }
  if (o.want_centroids) K4_TRY(r.snp_centroid_file());
  k4_snp_files& f = out->files;
  if (o.want_wig)  // :8235
    K4_TRY(r.wig.finish(ix, "track type=wiggle_0 name=\"Coverage\" description=\"Alignment Segment Coverage\" useScore=1\n", hand, &f.wig, &f.wig_bytes));
  K4_TRY(hand.give(ix, &f.snp, &f.snp_bytes, r.text));
  if (o.want_hap) {
    K4_TRY(hand.give(ix, &f.disnp, &f.disnp_bytes, r.di));
    K4_TRY(hand.give(ix, &f.trisnp, &f.trisnp_bytes, r.tri));
  }
  if (o.marker_len) K4_TRY(hand.give(ix, &out->markers, &out->markers_bytes, r.markers));
  if (o.want_centroids) K4_TRY(hand.give(ix, &out->centroids, &out->centroids_bytes, r.centroids));
  f.n_snps = r.tot_snps;
  out->n_markers = r.n_markers;
  return hand.ok();
}

}  // namespace

// the SNP file alone or with the WIG, into the caller's pointers: what k4_snp_csv_dev, k4_snp_vcf_dev and k4_snp_files_dev hand out
static int snp_text(k4_index* ix, const K4Records& rec, const SnpOpts& o, char** snp, uint64_t* snp_bytes, uint64_t* n_snps, char** wig, uint64_t* wig_bytes,
                    void* stream) {
  if (!snp || !snp_bytes || (o.want_wig && (!wig || !wig_bytes))) return K4_ERR_PARAMS;
  k4_snp_files2 f;
  const int rc = snp_files(ix, rec, o, &f, stream);  // (an error leaves f zeroed)
  *snp = f.files.snp; *snp_bytes = f.files.snp_bytes;
  if (n_snps) *n_snps = f.files.n_snps;
  if (o.want_wig) { *wig = f.files.wig; *wig_bytes = f.files.wig_bytes; }
  return rc;
}
extern "C" int k4_snp_csv_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                              const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens, int32_t min_snp_reads,
                              double qvalue, double snp_nonref_pcnt, char** csv, uint64_t* csv_bytes, uint64_t* n_snps, void* stream) {
  return snp_text(ix, K4Records{pe, n_units, d_rr, d_hits, max_ml, d_pe, d_reads, d_offs, d_lens}, SnpOpts{0, min_snp_reads, qvalue, snp_nonref_pcnt, false, false},
                  csv, csv_bytes, n_snps, nullptr, nullptr, stream);
}
// the VCF form (kalign: a SNP file name ending in .vcf, KAligner.cpp:186-187; header :8196-8199, records :7650-7696)
extern "C" int k4_snp_vcf_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                              const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens, int32_t min_snp_reads,
                              double qvalue, double snp_nonref_pcnt, char** vcf, uint64_t* vcf_bytes, uint64_t* n_snps, void* stream) {
  return snp_text(ix, K4Records{pe, n_units, d_rr, d_hits, max_ml, d_pe, d_reads, d_offs, d_lens}, SnpOpts{1, min_snp_reads, qvalue, snp_nonref_pcnt, false, false},
                  vcf, vcf_bytes, n_snps, nullptr, nullptr, stream);
}
// both files of a kalign SNP run: the SNP file (CSV, or VCF when vcf != 0) and the coverage WIG (<snp file>.covsegs.wig)
extern "C" int k4_snp_files_dev(k4_index* ix, int vcf, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                                const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens, int32_t min_snp_reads,
                                double qvalue, double snp_nonref_pcnt, char** snp, uint64_t* snp_bytes, uint64_t* n_snps, char** wig,
                                uint64_t* wig_bytes, void* stream) {
  return snp_text(ix, K4Records{pe, n_units, d_rr, d_hits, max_ml, d_pe, d_reads, d_offs, d_lens}, SnpOpts{vcf, min_snp_reads, qvalue, snp_nonref_pcnt, true, false},
                  snp, snp_bytes, n_snps, wig, wig_bytes, stream);
}
// every file of a kalign SNP run: the SNP file, the coverage WIG and the two haplotype files (.disnp.csv, .trisnp.csv)
extern "C" int k4_snp_run_dev(k4_index* ix, int vcf, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                              const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens, int32_t min_snp_reads,
                              double qvalue, double snp_nonref_pcnt, k4_snp_files* out, void* stream) {
  if (!out) return K4_ERR_PARAMS;
  k4_snp_files2 f;
  const int rc = snp_files(ix, K4Records{pe, n_units, d_rr, d_hits, max_ml, d_pe, d_reads, d_offs, d_lens},
                           SnpOpts{vcf, min_snp_reads, qvalue, snp_nonref_pcnt, true, true}, &f, stream);
  *out = f.files;  // (an error leaves f zeroed)
  return rc;
}
// ... and, as the options ask, the marker sequences (<snp file>.markers) and the SNP centroid distribution
extern "C" int k4_snp_run2_dev(k4_index* ix, int vcf, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                               const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens, int32_t min_snp_reads,
                               double qvalue, double snp_nonref_pcnt, const k4_snp_opts* opts, k4_snp_files2* out, void* stream) {
  if (!out || !opts) return K4_ERR_PARAMS;
  return snp_files(ix, K4Records{pe, n_units, d_rr, d_hits, max_ml, d_pe, d_reads, d_offs, d_lens},
                   SnpOpts{vcf, min_snp_reads, qvalue, snp_nonref_pcnt, true, true, opts->marker_len, opts->marker_poly_thres, opts->want_centroids != 0}, out, stream);
}
// the marker rule alone, on the host: no device, no index.  cnt7: seven arrays of `stride` words each (ref, nonref, A, C, G, T, N);
// base[l] = 0..4, or 0xff (coverage below min_snp_reads) / 0xfe (no allele reaches 1 - threshold); poly[l] = 1 for a polymorphic locus
extern "C" int k4_marker_classify_host(const uint32_t* cnt7, uint64_t stride, uint32_t n_loci, const uint8_t* ref_bases, int32_t min_snp_reads,
                                       double poly_thres, uint8_t* base, uint8_t* poly) {
  if ((!cnt7 || !ref_bases || !base || !poly) && n_loci) return K4_ERR_PARAMS;
  if (stride < n_loci || min_snp_reads < 1) return K4_ERR_PARAMS;
  for (uint32_t l = 0; l < n_loci; l++) {
    const uint32_t by_base[5] = {cnt7[2 * stride + l], cnt7[3 * stride + l], cnt7[4 * stride + l], cnt7[5 * stride + l], cnt7[6 * stride + l]};
    int p = 0;
    const int b = k4_marker_base(cnt7[l], cnt7[stride + l], by_base, ref_bases[l], min_snp_reads, poly_thres, &p);
    base[l] = b == K4_MARKER_NO_COVERAGE ? 0xff : b == K4_MARKER_NO_ALLELE ? 0xfe : (uint8_t)b;
    poly[l] = (uint8_t)p;
  }
  return K4_OK;
}
extern "C" void k4_free_host(void* p) { free(p); }
