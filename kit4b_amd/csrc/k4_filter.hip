// kit4b_amd/csrc/k4_filter.hip -- the kalign options that decide which accepted alignments are kept, over the records the align
// calls (and the stages behind them) left in HBM:
//   k4_filter_loci_constraints_dev <- CKAligner::IdentifyConstraintViolations  ngskit4b/KAligner.cpp:2716-2765   (`kalign -5 <file>`)
//                                     AcceptLociConstraints :2647-2714, AcceptBaseConstraint :2598-2645
//   k4_filter_chroms_dev           <- CKAligner::FiltByChroms :4025-4091        (`kalign -Z <regex>` / `-z <regex>`)
//   k4_load_loci_constraints       <- CKAligner::LoadLociConstraints :1363-1545 over CCSVFile (libkit4b/CSVFile.cpp)   [host]
//   k4_chrom_accept_mask           <- CUtility::CompileREs / MatchExcludeRegExpr / MatchIncludeRegExpr (libkit4b/Utility.cpp:78-287) [host]
//
// Loci constraints.  The reference walks every base of every accepted read on a constrained sequence past the whole constraint list.
// What it computes is one bit per read -- "some locus of the read lies inside a constraint that its base does not satisfy" -- so here:
//   * the table, sorted by (sequence, start, end), sits in LDS with the running maximum of `end` beside it (the constraints that
//     overlap [s, e] are then found by two binary searches: the first one whose running maximum reaches s, the last one that starts
//     at or before e), together with the (at most 64) constrained sequences and their slices of the table;
//   * phase A, a lane per read: accepted? on a constrained sequence? does a constraint overlap one of its segments?
//   * phase B, the wave per read that passed A, lanes over the read's positions: the base of the read (reverse complemented for a
//     Crick alignment) against every constraint of the slice that covers the locus; `R` fetches the target base from the packed
//     sequence.  One __any() per segment gives the read's bit.
// A read that fails becomes K4_NAR_LOCICONSTRAINED with NumHits = LowHitInstances = 0; PE: so does its mate, whatever its state.
// Mates are neighbours (reads 2i, 2i + 1), hence neighbouring lanes of one wave: every lane writes its own record only.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <regex>
#include <string>
#include <vector>
#include "k4_device.h"
#include "k4_stage.h"

#define K4_MAX_CONSTRAINED_CHROMS 64                                 /* cMaxConstrainedChroms, KAligner.h:92 */
#define K4_MAX_CONSTRAINED_LOCI (K4_MAX_CONSTRAINED_CHROMS * 100)    /* cMaxConstrainedLoci, KAligner.h:93 */
#define K4_MAX_CHROM_RES 20                                          /* cMaxIncludeChroms / cMaxExcludeChroms, KAligner.h:33-34 */
#define K4_MAX_LEN_RE 100                                            /* cMaxLenRE, libkit4b/Utility.h:4 */
#define K4_FILTER_THREADS 1024                                       /* one block per CU holds the table once for 16 waves */

namespace {

// first k in [lo, hi) with a[k] > v (upper) / a[k] >= v (lower); a ascending
K4_DEV uint32_t k4d_first_gt(const uint32_t* a, uint32_t lo, uint32_t hi, uint32_t v) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
K4_DEV uint32_t k4d_first_ge(const uint32_t* a, uint32_t lo, uint32_t hi, uint32_t v) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The table as the host lays it out (32-bit words): start[n] | end[n] | running max of end within the sequence [n] |
// {sequence id, first, one past last}[nc] | the constraint bytes, four to a word.
__global__ void __launch_bounds__(K4_FILTER_THREADS)
k4k_filter_loci(K4DevIndex ix, const uint32_t* __restrict__ g_tab, uint32_t n_c, uint32_t n_ch, uint32_t tab_words, K4ReadSet rs,
                unsigned long long* __restrict__ n_marked) {
  extern __shared__ uint32_t lds[];
  for (uint32_t k = threadIdx.x; k < tab_words; k += K4_FILTER_THREADS) lds[k] = g_tab[k];
  __syncthreads();
  const uint32_t* c_start = lds;
  const uint32_t* c_end = lds + n_c;
  const uint32_t* c_pmax = lds + 2 * n_c;
  const uint32_t* c_chrom = lds + 3 * n_c;
  const uint8_t* c_bits = reinterpret_cast<const uint8_t*>(lds + 3 * n_c + 3 * n_ch);
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (K4_FILTER_THREADS / 64) + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * (K4_FILTER_THREADS / 64);
  const int64_t n_reads = rs.n_reads;
  uint32_t marked = 0;
  for (int64_t base = wave * 64; base < n_reads; base += n_waves * 64) {  // (base is wave-uniform: the wave stays together)
    const int64_t i = base + lane;
    // ---- phase A: a lane per read
    int32_t nar = -1;
    k4_hit h = {0, 0, 0, 0, 0, 0};
    uint32_t seg_s[2] = {0, 0}, seg_e[2] = {0, 0}, seg_q[2] = {0, 0}, seg_k0[2] = {0, 0}, seg_k1[2] = {0, 0};
    uint32_t rlen = 0, off_lo = 0, off_hi = 0;
    if (i < n_reads) {
      nar = rs.nar(i);
      if (nar == K4_NAR_ACCEPTED) {
        h = rs.hit(i);
        uint32_t lo = 0, hi = n_ch;  // the sequence among the constrained ones (m_ConstrainedChromIDs)
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (c_chrom[3 * mid] < h.chrom_id) lo = mid + 1; else hi = mid;
        }
        if (lo < n_ch && c_chrom[3 * lo] == h.chrom_id && h.chrom_id >= 1 && h.chrom_id <= ix.n_entries) {
          const uint32_t t_lo = c_chrom[3 * lo + 1], t_hi = c_chrom[3 * lo + 2];
          // Seg[0]: AdjStartLoci .. AdjEndLoci; the walk of the read starts at ReadOfs (0) + TrimLeft on either strand
          if ((int32_t)k4d_adj_len(h) > 0) {
            seg_s[0] = k4d_adj_start(h);
            seg_e[0] = k4d_adj_end(h);
            seg_q[0] = K4_HIT_TRIM_LEFT(h);
            seg_k1[0] = k4d_first_gt(c_start, t_lo, t_hi, seg_e[0]);
            seg_k0[0] = k4d_first_ge(c_pmax, t_lo, seg_k1[0], seg_s[0]);
          }
          if ((h.ext & (K4_EXT_INDEL | K4_EXT_SPLICE)) && rs.seg2) {  // FlagSegs: Seg[1] (no trims of its own)
            const k4_seg2 s2 = rs.seg2[i];
            if (s2.match_len) {
              seg_s[1] = s2.match_loci;
              seg_e[1] = s2.match_loci + (uint32_t)s2.match_len - 1u;
              seg_q[1] = s2.read_ofs;
              seg_k1[1] = k4d_first_gt(c_start, t_lo, t_hi, seg_e[1]);
              seg_k0[1] = k4d_first_ge(c_pmax, t_lo, seg_k1[1], seg_s[1]);
            }
          }
          if (seg_k0[0] < seg_k1[0] || seg_k0[1] < seg_k1[1]) {
            const uint64_t o = rs.offs[i];
            off_lo = (uint32_t)o; off_hi = (uint32_t)(o >> 32);
            rlen = rs.lens[i];
          }
        }
      }
    }
    // ---- phase B: the wave per read that a constraint overlaps
    bool viol = false;
    unsigned long long todo = __ballot(seg_k0[0] < seg_k1[0] || seg_k0[1] < seg_k1[1]);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const uint32_t b_len = __shfl(rlen, src, 64);
      const uint8_t* rd = rs.reads + (((uint64_t)__shfl(off_hi, src, 64) << 32) | __shfl(off_lo, src, 64));
      const bool b_minus = __shfl((int)h.strand, src, 64) == '-';
      const uint64_t b_cs = ix.ent_start[__shfl(h.chrom_id, src, 64) - 1];
      bool fail = false;
#pragma unroll
      for (int sg = 0; sg < 2; sg++) {
        const uint32_t k0 = __shfl(seg_k0[sg], src, 64), k1 = __shfl(seg_k1[sg], src, 64);
        if (k0 >= k1) continue;
        const uint32_t s = __shfl(seg_s[sg], src, 64), span = __shfl(seg_e[sg], src, 64) - s, q0 = __shfl(seg_q[sg], src, 64);
        for (uint32_t j = (uint32_t)lane; j <= span && !fail; j += 64u) {
          const uint32_t loci = s + j, q = q0 + j;
          uint32_t b = 4u;  // (a record whose walk leaves the read: an indeterminate base)
          if (q < b_len) {
            b = (b_minus ? rd[b_len - 1u - q] : rd[q]) & 7u;
            if (b_minus && b <= 3u) b = 3u - b;  // CSeqTrans::ReverseComplement leaves the other symbols as they are
          }
          uint32_t tb = 0xFFu;
          for (uint32_t k = k0; k < k1; k++) {
            if (c_start[k] > loci || c_end[k] < loci) continue;
            const uint32_t bits = c_bits[k];
            bool ok = false;
            if (bits & 0x10u) {  // R: the base of the target (an N in the read passes over an N only)
              if (tb == 0xFFu) tb = b_cs + loci < ix.n ? k4d_ref_base(ix, b_cs + loci) : 7u;
              ok = tb == b;
            }
            if (!ok) ok = b <= 3u && ((bits >> b) & 1u);
            if (!ok) { fail = true; break; }
          }
        }
      }
      if (__any(fail) && lane == src) viol = true;
    }
    // ---- the marks: every lane its own record; PE mates are lanes 2q, 2q + 1
    bool lc = viol;
    if (rs.pe()) {
      lc = lc || nar == K4_NAR_LOCICONSTRAINED;
      const int mate = __shfl_xor((int)lc, 1, 64);  // (every lane takes part: no short circuit in front of the shuffle)
      lc = lc || mate != 0;
    }
    const bool fresh = lc && i < n_reads && nar != K4_NAR_LOCICONSTRAINED;
    if (fresh) rs.reject(i, K4_NAR_LOCICONSTRAINED, true);  // NAR, NumHits and LowHitInstances (:2736-2738, the mate :2753-2755)
    // (PE: a mate that was not accepted is tallied by the NAR it loses; few of them)
    if (fresh && nar != K4_NAR_ACCEPTED && nar >= 0 && nar < 20) atomicAdd(n_marked + 1 + nar, 1ull);
    marked += (uint32_t)__popcll(__ballot(fresh));
  }
  if (lane == 0 && marked) atomicAdd(n_marked, (unsigned long long)marked);
}

// FiltByChroms: an accepted read on a sequence the expressions reject
__global__ void __launch_bounds__(256) k4k_filter_chroms(uint32_t n_entries, const uint8_t* __restrict__ accept, K4ReadSet rs,
                                                         unsigned long long* __restrict__ n_marked) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t n_reads = rs.n_reads;
  uint32_t marked = 0;
  for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); base < n_reads; base += stride) {
    const int64_t i = base + lane;
    bool drop = false;
    if (i < n_reads) {
      if (rs.nar(i) == K4_NAR_ACCEPTED) {
        const uint32_t c = rs.hit(i).chrom_id;
        drop = c >= 1 && c <= n_entries && accept[c] == 0;
      }
    }
    if (drop) rs.reject(i, K4_NAR_CHROMFILT, true);  // NAR, NumHits and LowHitInstances (:4058-4060, :4074-4076)
    marked += (uint32_t)__popcll(__ballot(drop));
  }
  if (lane == 0 && marked) atomicAdd(n_marked, (unsigned long long)marked);
}

int grid_for(int device, int per_cu) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
  return cus * per_cu;
}

}  // namespace

extern "C" int k4_filter_chroms_dev(k4_index* ix, const void* d_accept, int pe, int64_t n_reads, int32_t max_ml, void* d_rr_or_pe,
                                    const void* d_hits, int64_t* n_removed, void* stream) {
  if (!ix) return K4_ERR_PARAMS;
  if (n_removed) *n_removed = 0;
  if (n_reads <= 0) return K4_OK;
  K4ReadSet rs;
  K4_TRY(k4s_read_set(ix, pe, n_reads, d_rr_or_pe, d_hits, max_ml, d_rr_or_pe, nullptr, nullptr, nullptr, nullptr, K4RS_HITS, &rs));
  if (!d_accept) return k4_fail(ix, K4_ERR_PARAMS, "null buffer");
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  K4DevBuf cnt;
  K4_HIP(ix, cnt.alloc(8));
  K4_HIP(ix, hipMemsetAsync(cnt.p, 0, 8, st));
  const int64_t blocks = std::min<int64_t>((n_reads + 255) / 256, grid_for(ix->device, 8));
  hipLaunchKernelGGL(k4k_filter_chroms, dim3((unsigned)blocks), dim3(256), 0, st, ix->d.n_entries, (const uint8_t*)d_accept, rs,
                     cnt.as<unsigned long long>());
  K4_HIP(ix, hipGetLastError());
  unsigned long long c = 0;
  K4_TRY(k4s_read_back(ix, &c, cnt.p, st));
  if (n_removed) *n_removed = (int64_t)c;
  ix->filter_prior[K4_NAR_ACCEPTED] += c;
  return K4_OK;
}

extern "C" int k4_filter_marked_prior(const k4_index* ix, uint64_t* prior20) {
  if (!ix || !prior20) return K4_ERR_PARAMS;
  memcpy(prior20, ix->filter_prior, sizeof(ix->filter_prior));
  return K4_OK;
}

extern "C" int k4_filter_loci_constraints_dev(k4_index* ix, const k4_loci_constraint* constraints, int32_t n_constraints, int pe,
                                              int64_t n_units, int32_t max_ml, void* d_rr, const void* d_hits, const void* d_seg2,
                                              void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens,
                                              int64_t* n_removed, void* stream) {
  if (!ix) return K4_ERR_PARAMS;
  if (n_removed) *n_removed = 0;
  if (n_constraints < 0 || n_constraints > K4_MAX_CONSTRAINED_LOCI)
    return k4_fail(ix, K4_ERR_PARAMS, "%d loci base constraints, at most %d are allowed", (int)n_constraints, K4_MAX_CONSTRAINED_LOCI);
  if (n_constraints == 0 || n_units <= 0) return K4_OK;  // "there may be no constraints!"
  K4ReadSet rs;
  K4_TRY(k4s_read_set(ix, pe, n_units, d_rr, d_hits, max_ml, d_pe, d_seg2, d_reads, d_offs, d_lens, K4RS_HITS | K4RS_READS | K4RS_UNITS, &rs));
  if (!constraints) return k4_fail(ix, K4_ERR_PARAMS, "null buffer");
  // the table: checked, sorted by (sequence, start, end) as the reference sorts it, with the running maximum of `end`
  std::vector<k4_loci_constraint> t(constraints, constraints + n_constraints);
  for (const k4_loci_constraint& c : t) {
    if (c.chrom_id < 1 || c.chrom_id > ix->entries.size()) return k4_fail(ix, K4_ERR_PARAMS, "loci base constraint on sequence %u: no such sequence", c.chrom_id);
    if (c.start > c.end || c.end >= ix->entries[c.chrom_id - 1].seq_len)
      return k4_fail(ix, K4_ERR_PARAMS, "loci base constraint %u..%u outside of sequence %u", c.start, c.end, c.chrom_id);
    if (c.bits == 0 || (c.bits & ~0x1Fu)) return k4_fail(ix, K4_ERR_PARAMS, "loci base constraint with base bits 0x%02x", (unsigned)c.bits);
  }
  std::stable_sort(t.begin(), t.end(), [](const k4_loci_constraint& a, const k4_loci_constraint& b) {
    return a.chrom_id != b.chrom_id ? a.chrom_id < b.chrom_id : a.start != b.start ? a.start < b.start : a.end < b.end;
  });
  const uint32_t n = (uint32_t)n_constraints;
  std::vector<uint32_t> chrom;
  for (uint32_t k = 0; k < n; k++) {
    if (k == 0 || t[k].chrom_id != t[k - 1].chrom_id) { if (!chrom.empty()) chrom.back() = k; chrom.insert(chrom.end(), {t[k].chrom_id, k, n}); }
  }
  const uint32_t nc = (uint32_t)chrom.size() / 3;
  if (nc > K4_MAX_CONSTRAINED_CHROMS)
    return k4_fail(ix, K4_ERR_PARAMS, "loci base constraints on %u sequences, at most %d are allowed", nc, K4_MAX_CONSTRAINED_CHROMS);
  const uint32_t words = 3 * n + 3 * nc + (n + 3) / 4;
  std::vector<uint32_t> tab(words, 0);
  for (uint32_t k = 0; k < n; k++) {
    tab[k] = t[k].start;
    tab[n + k] = t[k].end;
    tab[2 * n + k] = (k && t[k].chrom_id == t[k - 1].chrom_id) ? std::max(tab[2 * n + k - 1], t[k].end) : t[k].end;
    reinterpret_cast<uint8_t*>(tab.data() + 3 * n + 3 * nc)[k] = t[k].bits;
  }
  std::copy(chrom.begin(), chrom.end(), tab.begin() + 3 * n);
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  K4DevBuf d_tab, cnt;  // cnt: [0] reads marked, [1 + k] those of them that carried NAR k and were not accepted
  K4_HIP(ix, d_tab.alloc((size_t)words * 4));
  K4_HIP(ix, cnt.alloc(8 * 21));
  K4_HIP(ix, hipMemcpyAsync(d_tab.p, tab.data(), (size_t)words * 4, hipMemcpyHostToDevice, st));
  K4_HIP(ix, hipMemsetAsync(cnt.p, 0, 8 * 21, st));
  const size_t lds = (size_t)words * 4;  // at most 84 KB of the CU's 160
  K4_HIP(ix, hipFuncSetAttribute((const void*)k4k_filter_loci, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t blocks = std::min<int64_t>((rs.n_reads + K4_FILTER_THREADS - 1) / K4_FILTER_THREADS, grid_for(ix->device, 1));
  hipLaunchKernelGGL(k4k_filter_loci, dim3((unsigned)blocks), dim3(K4_FILTER_THREADS), lds, st, ix->d, d_tab.as<uint32_t>(), n, nc, words, rs,
                     cnt.as<unsigned long long>());
  K4_HIP(ix, hipGetLastError());
  unsigned long long c[21];
  K4_TRY(k4s_read_back(ix, &c, cnt.p, st));  // (the host copy of the table is read by the upload until here)
  if (n_removed) *n_removed = (int64_t)c[0];
  unsigned long long others = 0;
  for (int k = 0; k < 20; k++) { ix->filter_prior[k] += c[1 + k]; others += c[1 + k]; }
  ix->filter_prior[K4_NAR_ACCEPTED] += c[0] - others;
  return K4_OK;
}

// ---- host side: the constraints file and the expressions -------------------------------------------------------------------------
namespace {

struct CsvField { std::string v; bool quoted = false; };

// one line of a CCSVFile (libkit4b/CSVFile.cpp: ParseField): comma separated, blanks around a value dropped, a value may be quoted
std::vector<CsvField> csv_fields(const std::string& line) {
  std::vector<CsvField> out;
  size_t p = 0;
  for (;;) {
    CsvField f;
    while (p < line.size() && (line[p] == ' ' || line[p] == '\t')) p++;
    if (p < line.size() && (line[p] == '"' || line[p] == '\'')) {
      const char q = line[p++];
      while (p < line.size() && line[p] != q) f.v += line[p++];
      if (p < line.size()) p++;
      f.quoted = true;
      while (p < line.size() && line[p] != ',') p++;
    } else {
      while (p < line.size() && line[p] != ',') f.v += line[p++];
      while (!f.v.empty() && (f.v.back() == ' ' || f.v.back() == '\t')) f.v.pop_back();
    }
    out.push_back(f);
    if (p >= line.size()) break;
    p++;  // the separator
  }
  return out;
}

// CCSVFile::IsLikelyHeaderLine (:762-789): at most two empty fields, every other one quoted or not a number
bool likely_header(const std::vector<CsvField>& f) {
  int empty = 0;
  for (const CsvField& x : f) {
    if (x.quoted) continue;
    if (x.v.empty()) { if (++empty > 2) return false; continue; }
    char* term = nullptr;
    (void)strtod(x.v.c_str(), &term);
    if (term && *term == '\0') return false;
  }
  return true;
}

int load_fail(k4_index* ix, char* errbuf, int code, const char* fmt, ...) {
  char msg[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof(msg), fmt, ap);
  va_end(ap);
  if (errbuf) { strncpy(errbuf, msg, 255); errbuf[255] = 0; }
  return k4_fail(ix, code, "%s", msg);
}

}  // namespace

extern "C" int k4_load_loci_constraints(k4_index* ix, const char* path, k4_loci_constraint** tbl, int32_t* n, char* errbuf) {
  if (!ix || !path || !tbl || !n) return K4_ERR_PARAMS;
  *tbl = nullptr;
  *n = 0;
  if (errbuf) errbuf[0] = 0;
  FILE* fp = fopen(path, "rb");
  if (!fp) return load_fail(ix, errbuf, K4_ERR_OPEN_FILE, "Unable to open '%s' for processing", path);
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) text.append(buf, got);
  fclose(fp);
  std::vector<k4_loci_constraint> t;
  std::vector<uint32_t> chroms;
  std::string prev;
  int chrom_id = 0, n_lines = 0, line_no = 0;
  for (size_t p = 0; p < text.size();) {
    size_t e = text.find_first_of("\r\n", p);
    if (e == std::string::npos) e = text.size();
    std::string line = text.substr(p, e - p);
    p = e;
    if (p < text.size()) { if (text[p] == '\r' && p + 1 < text.size() && text[p + 1] == '\n') p++; p++; }
    line_no++;
    size_t a = line.find_first_not_of(" \t");
    if (a == std::string::npos || line[a] == '#') continue;  // blank lines and comment lines are sloughed (CCSVFile::NextLine)
    const std::vector<CsvField> f = csv_fields(line.substr(a));
    n_lines++;
    if (f.size() < 4)
      return load_fail(ix, errbuf, K4_ERR_PARSE, "Expected at least 4 fields at line %d in '%s', GetCurFields() returned '%d'", line_no, path, (int)f.size());
    if (n_lines == 1 && likely_header(f)) continue;
    const std::string& name = f[0].v;
    const int start = atoi(f[1].v.c_str()), end = atoi(f[2].v.c_str());
    if (chrom_id == 0 || prev.empty() || strcasecmp(name.c_str(), prev.c_str())) {
      prev = name.substr(0, 79);
      if ((chrom_id = k4_get_ident(ix, prev.c_str())) <= 0)
        return load_fail(ix, errbuf, K4_ERR_PARSE, "Unable to find matching indexed identifier for '%s' at line %d in '%s'", prev.c_str(), line_no, path);
    }
    if (start < 0 || start > end)
      return load_fail(ix, errbuf, K4_ERR_PARSE, "Start loci must be >= 0 and <= end loci for '%s' at line %d in '%s'", prev.c_str(), line_no, path);
    if ((uint32_t)end >= ix->entries[(size_t)chrom_id - 1].seq_len)
      return load_fail(ix, errbuf, K4_ERR_PARSE, "End loci must be > targeted sequence length for '%s' at line %d in '%s'", prev.c_str(), line_no, path);
    uint8_t bits = 0;
    bool bad = false;
    for (const char ch : f[3].v) {
      switch (ch) {
        case 'a': case 'A': bits |= 0x01; break;
        case 'c': case 'C': bits |= 0x02; break;
        case 'g': case 'G': bits |= 0x04; break;
        case 't': case 'T': bits |= 0x08; break;
        case 'r': case 'R': bits |= 0x10; break;
        case ' ': case '\t': break;
        default: bad = true;
      }
    }
    if (bad || bits == 0)
      return load_fail(ix, errbuf, K4_ERR_PARSE, "Illegal base specifiers for '%s' at line %d in '%s'", prev.c_str(), line_no, path);
    if (std::find(chroms.begin(), chroms.end(), (uint32_t)chrom_id) == chroms.end()) {
      if (chroms.size() == K4_MAX_CONSTRAINED_CHROMS)
        return load_fail(ix, errbuf, K4_ERR_PARSE, "Number of constrained chroms would be more than max (%d) allowed for '%s' at line %d in '%s'",
                         K4_MAX_CONSTRAINED_CHROMS, prev.c_str(), line_no, path);
      chroms.push_back((uint32_t)chrom_id);
    }
    if (t.size() == K4_MAX_CONSTRAINED_LOCI)
      return load_fail(ix, errbuf, K4_ERR_PARSE, "Number of constrained loci would be more than max (%d) allowed for '%s' at line %d in '%s'",
                       K4_MAX_CONSTRAINED_LOCI, prev.c_str(), line_no, path);
    k4_loci_constraint c;
    memset(&c, 0, sizeof(c));
    c.chrom_id = (uint32_t)chrom_id; c.start = (uint32_t)start; c.end = (uint32_t)end; c.bits = bits;
    t.push_back(c);
  }
  std::stable_sort(t.begin(), t.end(), [](const k4_loci_constraint& a, const k4_loci_constraint& b) {
    return a.chrom_id != b.chrom_id ? a.chrom_id < b.chrom_id : a.start != b.start ? a.start < b.start : a.end < b.end;
  });
  if (!t.empty()) {
    *tbl = (k4_loci_constraint*)malloc(t.size() * sizeof(k4_loci_constraint));
    if (!*tbl) return load_fail(ix, errbuf, K4_ERR_MEM, "out of memory for %zu loci base constraints", t.size());
    memcpy(*tbl, t.data(), t.size() * sizeof(k4_loci_constraint));
  }
  *n = (int32_t)t.size();
  return K4_OK;
}

extern "C" int k4_chrom_accept_mask(k4_index* ix, int32_t n_incl, const char* const* incl, int32_t n_excl, const char* const* excl, uint8_t* mask) {
  if (!ix || !mask || n_incl < 0 || n_excl < 0 || (n_incl && !incl) || (n_excl && !excl)) return K4_ERR_PARAMS;
  if (n_incl > K4_MAX_CHROM_RES || n_excl > K4_MAX_CHROM_RES)
    return k4_fail(ix, K4_ERR_PARAMS, "at most %d chromosome expressions of either kind", K4_MAX_CHROM_RES);
  std::vector<std::regex> re[2];
  for (int which = 0; which < 2; which++) {
    const int cnt = which ? n_excl : n_incl;
    for (int k = 0; k < cnt; k++) {
      // TrimQuotedWhitespcExtd (KAlignerCL.cpp:1003-1019): blanks and one pair of quotes around the expression go; cMaxLenRE characters are kept
      std::string s = (which ? excl : incl)[k] ? (which ? excl : incl)[k] : "";
      auto trim = [&] {
        while (!s.empty() && (s.back() == ' ' || s.back() == '\t')) s.pop_back();
        size_t a = 0;
        while (a < s.size() && (s[a] == ' ' || s[a] == '\t')) a++;
        s.erase(0, a);
      };
      trim();
      if (s.size() >= 2 && (s.front() == '"' || s.front() == '\'') && s.back() == s.front()) { s = s.substr(1, s.size() - 2); trim(); }
      s = s.substr(0, K4_MAX_LEN_RE);
      try {
        re[which].emplace_back(s);  // the default (ECMAScript) grammar, as `new regex(szRE)`
      } catch (const std::regex_error& err) {
        return k4_fail(ix, K4_ERR_PARAMS, "Unable to compile %s regular expression '%s' - '%s'", which ? "exclusion" : "inclusion", s.c_str(), err.what());
      }
    }
  }
  mask[0] = 0;
  for (size_t c = 0; c < ix->entries.size(); c++) {
    std::string name = ix->entries[c].name;  // the name up to its first blank, cMaxLenRE characters at most
    name = name.substr(0, std::min<size_t>(name.find_first_of(" \t"), K4_MAX_LEN_RE));
    bool keep = true;
    for (const std::regex& r : re[1]) if (std::regex_search(name, r)) { keep = false; break; }
    if (keep && !re[0].empty()) {
      keep = false;
      for (const std::regex& r : re[0]) if (std::regex_search(name, r)) { keep = true; break; }
    }
    mask[c + 1] = keep ? 1 : 0;
  }
  return K4_OK;
}
