// kit4b_amd/csrc/k4_contam.hip -- kalign's contaminant flank trimming (`-H <file>`, --contaminants) as an ingest stage.
//   k4_load_contaminants   <- CContaminants::LoadContaminantsFile libkit4b/Contaminants.cpp:211-443, AddFlankContam :650-816   [host]
//   k4_contam_match_host   <- CContaminants::MatchContaminants :1243-1325 as the rule of k4_contam_rule.h                      [host]
//   k4_contam_trims_dev    <- the four MatchContaminants calls per read / pair of CKAligner::LoadRawReads
//                             ngskit4b/KAligner.cpp:11992-12039, for every read of a parsed chunk
// The reference walks a trie per overlap length; the kernel takes the rule the trie answers (k4_contam_rule.h) and tries every
// (contaminant, overlap length) of a read end directly: one wave per read end, the lanes split that space, longest overlaps
// first, and the wave stops at the first step in which a lane accepts.  A class's table (at most K4_CONTAM_TILE entries at a time)
// is staged in LDS once per block, plane- and word-major so that neighbouring lanes read neighbouring 8-byte words.
#include <ctype.h>
#include <stdarg.h>
#include <string.h>
#include <strings.h>
#include <zlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "k4_contam_rule.h"
#include "k4_internal.h"

// ---- host: the contaminants file --------------------------------------------------------------------------------------------------
namespace {

int contam_fail(k4_index* ix, char* errbuf, int code, const char* fmt, ...) {
  char msg[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof(msg), fmt, ap);
  va_end(ap);
  if (errbuf) { strncpy(errbuf, msg, 255); errbuf[255] = 0; }
  return k4_fail(ix, code, "%s", msg);
}

const char* const kContamTypeTxt[4] = {"5'SE/PE1", "5'PE2", "3'SE/PE1", "3'PE2"};  // ContaminateType2Txt :508-533

struct ContamEntry {
  int cls;
  bool revcpl;
  std::string name;
  std::vector<uint8_t> bases;  // 0..4
};

struct ContamLoader {
  k4_index* ix;
  char* errbuf;
  const char* path;
  std::vector<ContamEntry> all;
  int seq_id = 0;
  std::string name;
  bool flag[8] = {false, false, false, false, false, false, false, false};
  bool is_vector = false;

  void default_classes() { flag[0] = flag[1] = flag[4] = flag[5] = true; }  // 5' of PE1 and PE2, as read and reverse complemented

  // a descriptor line (:274-348): its first word is the name, an `@` / `&` and digits 1..8 behind it the classes
  void descriptor(std::string d) {
    for (bool& f : flag) f = false;
    seq_id++;
    d = d.substr(0, 105);  // szDescription
    size_t a = d.find_first_not_of(" \t\r\n\v\f");
    if (a == std::string::npos) {
      name = "ContamSeq." + std::to_string(seq_id);
      default_classes();
      return;
    }
    name = d.substr(a, d.find_first_of(" \t\r\n\v\f", a) - a);
    // from the last character towards (not onto) the first: over digits 1..8, to the first character that is none
    size_t p = name.size() - 1;
    for (size_t idx = name.size(); idx > 1; idx--, p--)
      if (name[p] == '@' || name[p] == '&' || !(name[p] >= '1' && name[p] <= '8')) break;
    is_vector = name[p] == '&';
    if ((name[p] == '@' || name[p] == '&') && p + 1 < name.size()) {
      for (size_t q = p + 1; q < name.size(); q++) flag[name[q] - '1'] = true;
      name.resize(p);
    } else
      default_classes();
    name = name.substr(0, 80);  // cMaxGeneNameLen - 1
  }

  // AddFlankContam :650-816
  int add(int cls, bool revcpl, const std::string& nm, const std::vector<uint8_t>& bases) {
    if (nm.empty()) return contam_fail(ix, errbuf, K4_ERR_PARAMS, "AddFlankContam: Parameter errors");
    if (all.size() >= (size_t)K4_CONTAM_MAX_ENTRIES)
      return contam_fail(ix, errbuf, K4_ERR_PARAMS, "AddFlankContam: Too many flank contaminants (max allowed %d) current contaminant is '%s'",
                         K4_CONTAM_MAX_ENTRIES, nm.c_str());
    if (nm.size() > 80)
      return contam_fail(ix, errbuf, K4_ERR_PARSE, "AddFlankContam: Contaminant name '%s' of overlap type %s length must be <= %d ", nm.c_str(),
                         kContamTypeTxt[cls], 80);
    for (const ContamEntry& e : all) {
      if (e.cls != cls) continue;
      const bool same_seq = e.bases == bases, same_name = strcasecmp(e.name.c_str(), nm.c_str()) == 0;
      if (same_name)
        return contam_fail(ix, errbuf, K4_ERR_PARSE, "AddFlankContam: Contaminant name '%s' of overlap type %s duplicated with %s sequences", nm.c_str(),
                           kContamTypeTxt[cls], same_seq ? "same" : "different");
      if (same_seq)
        return contam_fail(ix, errbuf, K4_ERR_PARSE, "AddFlankContam: Contaminant names '%s' and '%s' of overlap type %s with duplicated sequence",
                           nm.c_str(), e.name.c_str(), kContamTypeTxt[cls]);
    }
    all.push_back({cls, revcpl, nm, bases});
    return K4_OK;
  }

  // the sequence behind a descriptor, or in front of the first one (:350-435)
  int record(const std::string& seq) {
    if (!seq_id) {
      seq_id = 1;
      name = "ContamSeq.1";
      for (bool& f : flag) f = false;
      default_classes();
    }
    if (is_vector)
      return contam_fail(ix, errbuf, K4_ERR_UNSUPPORTED, "vector contaminants ('&' codes: reads contained in '%s') are not built", name.c_str());
    if (seq.size() < (size_t)K4_CONTAM_MIN_LEN || seq.size() > (size_t)K4_CONTAM_MAX_LEN)
      return contam_fail(ix, errbuf, K4_ERR_PARSE, "LoadContamiantsFile: Sequence for '%s' outside of accepted length range %d..%d", name.c_str(),
                         K4_CONTAM_MIN_LEN, K4_CONTAM_MAX_LEN);
    std::vector<uint8_t> b(seq.size());
    for (size_t k = 0; k < seq.size(); k++) {  // CFasta::Ascii2Sense, Fasta.cpp:1657-1705
      switch (seq[k]) {
        case 'a': case 'A': b[k] = 0; break;
        case 'c': case 'C': b[k] = 1; break;
        case 'g': case 'G': b[k] = 2; break;
        case 't': case 'T': case 'u': case 'U': b[k] = 3; break;
        case '-':
          return contam_fail(ix, errbuf, K4_ERR_PARSE, "LoadContaminantsFile: Illegal base in %s sequence, only bases A,C,G,T,N accepted", name.c_str());
        default: b[k] = 4;
      }
    }
    int rc;
    for (int c = 0; c < 4; c++)
      if (flag[c] && (rc = add(c, false, name, b)) != K4_OK) return rc;
    if (flag[4] || flag[5] || flag[6] || flag[7]) {
      std::reverse(b.begin(), b.end());
      for (uint8_t& x : b) if (x < 4) x = 3 - x;
      const std::string rc_name = name + "xRC";
      for (int c = 0; c < 4; c++)
        if (flag[4 + c] && (rc = add(c, true, rc_name, b)) != K4_OK) return rc;
    }
    return K4_OK;
  }

  // the file as CFasta::ReadSequence hands it out (Fasta.cpp:1047-1187): '>' opens a descriptor wherever it stands, a descriptor ends
  // with its line, letters and '-' are sequence, everything else between them is sloughed; a descriptor without a sequence behind it
  // is given one base N
  int parse(const std::string& text) {
    std::string descr, seq;
    bool in_descr = false, owes_seq = false;
    int rc;
    for (size_t i = 0; i <= text.size(); i++) {
      const bool eof = i == text.size();
      unsigned char ch = eof ? '\n' : (unsigned char)text[i];
      if (!eof) {
        if (in_descr && ch > 0x7f) ch = '?';
        if ((ch < 0x20 || ch > 0x7f) && !(ch == '\n' || ch == '\r' || ch == '\t' || ch == ' '))
          return contam_fail(ix, errbuf, K4_ERR_FILE_ACCESS, "Errors whilst reading file - '%s' - illegal chr 0x%x", path, ch);
      }
      if (in_descr) {
        if (descr.empty() && (ch == ' ' || ch == '\t')) continue;
        if (ch == '\n' || ch == '\r') {
          descriptor(descr);
          in_descr = false;
          owes_seq = true;
        } else
          descr += (char)ch;
        if (!eof) continue;
      }
      if (eof || ch == '>') {
        if (!seq.empty()) { if ((rc = record(seq)) != K4_OK) return rc; }
        else if (owes_seq && (rc = record("N")) != K4_OK) return rc;
        seq.clear();
        owes_seq = false;
        if (!eof) { in_descr = true; descr.clear(); }
        continue;
      }
      if (ch == '-' || isalpha(ch)) seq += (char)ch;
    }
    return K4_OK;
  }
};

void pack_contaminant(const ContamEntry& e, k4_contaminant* c) {
  memset(c, 0, sizeof(*c));
  c->cls = (uint8_t)e.cls;
  c->len = (uint8_t)e.bases.size();
  c->revcpl = e.revcpl ? 1 : 0;
  const uint32_t at0 = e.cls < 2 ? 256u - (uint32_t)e.bases.size() : 0u;  // 5' classes: right aligned
  for (size_t k = 0; k < e.bases.size(); k++) {
    const uint32_t p = at0 + (uint32_t)k;
    const uint64_t bit = 1ull << (p & 63u);
    const uint8_t b = e.bases[k];
    if (b == 4) c->nmask[p >> 6] |= bit;
    else {
      if (b & 1) c->p0[p >> 6] |= bit;
      if (b & 2) c->p1[p >> 6] |= bit;
    }
  }
}

// the views k4_contam_subs reads through
struct HostContamView {
  const k4_contaminant* c;
  uint64_t word(uint32_t plane, uint32_t k) const { return plane == 0 ? c->p0[k] : plane == 1 ? c->p1[k] : plane == 2 ? c->nmask[k] : 0ull; }
};
struct HostReadView {
  uint64_t w[K4_CONTAM_PLANES][K4_CONTAM_WORDS];
  uint64_t word(uint32_t plane, uint32_t k) const { return w[plane][k]; }
};

}  // namespace

extern "C" int k4_load_contaminants(k4_index* ix, const char* path, k4_contaminant** tbl, int32_t* n, char* errbuf) {
  if (!path || !tbl || !n) return K4_ERR_PARAMS;
  *tbl = nullptr;
  *n = 0;
  if (errbuf) errbuf[0] = 0;
  gzFile fp = gzopen(path, "rb");  // (a file that is not gzip is read as it is)
  if (!fp) return contam_fail(ix, errbuf, K4_ERR_OPEN_FILE, "LoadContaminantsFile: Unable to open '%s'", path);
  std::string text;
  char buf[1 << 16];
  int got;
  while ((got = gzread(fp, buf, sizeof(buf))) > 0) {
    text.append(buf, (size_t)got);
    if (text.size() > (64u << 20)) break;  // (1600 entries of 200 bases: nothing the reference accepts comes near)
  }
  gzclose(fp);
  if (got < 0) return contam_fail(ix, errbuf, K4_ERR_FILE_ACCESS, "LoadContaminantsFile: Errors whilst reading file - '%s'", path);
  ContamLoader ld{ix, errbuf, path};
  const int rc = ld.parse(text);
  if (rc != K4_OK) return rc;
  if (ld.all.empty()) return contam_fail(ix, errbuf, K4_ERR_PARAMS, "FinaliseContaminant: No Contaminants loaded");
  // SortContamTypeLen: by class, longest first
  std::stable_sort(ld.all.begin(), ld.all.end(), [](const ContamEntry& a, const ContamEntry& b) {
    return a.cls != b.cls ? a.cls < b.cls : a.bases.size() > b.bases.size();
  });
  *tbl = (k4_contaminant*)malloc(ld.all.size() * sizeof(k4_contaminant));
  if (!*tbl) return contam_fail(ix, errbuf, K4_ERR_MEM, "out of memory for %zu contaminants", ld.all.size());
  for (size_t k = 0; k < ld.all.size(); k++) pack_contaminant(ld.all[k], *tbl + k);
  *n = (int32_t)ld.all.size();
  return K4_OK;
}

extern "C" int k4_contam_match_host(const k4_contaminant* tbl, int32_t n, int32_t cls, int32_t min_overlap, const uint8_t* read_bases,
                                    int32_t read_len) {
  if (n < 0 || (n && !tbl) || cls < 0 || cls > 3 || min_overlap < 0 || read_len < 0 || (read_len && !read_bases)) return K4_ERR_PARAMS;
  if (read_len < K4_CONTAM_MIN_READ || read_len > K4_CONTAM_MAX_READ) return 0;
  uint32_t longest = 0;
  for (int32_t k = 0; k < n; k++)
    if (tbl[k].cls == cls) longest = std::max<uint32_t>(longest, tbl[k].len);
  const uint32_t min_l = (uint32_t)std::max(min_overlap, 1), l_max = std::min<uint32_t>((uint32_t)read_len, longest);
  if (l_max < min_l) return 0;
  const bool five = cls < 2;
  HostReadView rv;
  memset(&rv, 0, sizeof(rv));
  for (uint32_t p = 0; p < 256u; p++) {
    const int64_t at = k4c_read_index(five, (uint32_t)read_len, p);
    if (at < 0) continue;
    const uint32_t planes = k4c_read_planes(read_bases[at]);
    for (uint32_t pl = 0; pl < (uint32_t)K4_CONTAM_PLANES; pl++)
      if (planes >> pl & 1u) rv.w[pl][p >> 6] |= 1ull << (p & 63u);
  }
  for (uint32_t L = l_max; L >= min_l; L--)
    for (int32_t k = 0; k < n; k++)
      if (tbl[k].cls == cls && tbl[k].len >= L && k4_contam_subs(rv, HostContamView{tbl + k}, L, five) <= 1u) return (int)L;
  return 0;
}

// ---- device -----------------------------------------------------------------------------------------------------------------------
#define K4_CONTAM_TILE 400     // entries of a class staged at a time: 12 rows of 8-byte words = 38.4 KB of the CU's 160 KB LDS
#define K4_CONTAM_THREADS 256  // four waves, one read end each
#define K4_CONTAM_ROWS 12      // planes 0..2 x words 0..3

namespace {

struct ContamClassArg {
  const uint64_t* bits;   // [K4_CONTAM_ROWS][n]
  const uint16_t* lens;   // [n], falling
  uint32_t n;
};

struct LdsContamView {
  const uint64_t* rows;  // s_bits
  uint32_t e;
  __device__ uint64_t word(uint32_t plane, uint32_t k) const { return plane < 3u ? rows[(plane * 4u + k) * K4_CONTAM_TILE + e] : 0ull; }
};
struct LdsReadView {
  const uint64_t* w;  // [plane][word]
  __device__ uint64_t word(uint32_t plane, uint32_t k) const { return w[plane * 4u + k]; }
};

// One read end per wave and trip.  out[unit * out_stride + out_ofs] = the overlap beyond `trim`; *tot += the units that got one.
__global__ void __launch_bounds__(K4_CONTAM_THREADS)
k4k_contam_trims(ContamClassArg cd, int five, int64_t n_units, int out_stride, int out_ofs, uint32_t trim, uint32_t sample_nth,
                 int64_t first_unit, const uint8_t* __restrict__ reads, const uint64_t* __restrict__ offs,
                 const uint32_t* __restrict__ lens, uint64_t base, uint8_t* __restrict__ out, unsigned long long* __restrict__ tot) {
  __shared__ uint64_t s_bits[K4_CONTAM_ROWS * K4_CONTAM_TILE];
  __shared__ uint16_t s_len[K4_CONTAM_TILE];
  __shared__ uint16_t s_cnt[K4_CONTAM_MAX_LEN + 2];  // s_cnt[L]: staged entries of at least L bases
  __shared__ uint64_t s_read[K4_CONTAM_THREADS / 64][K4_CONTAM_PLANES * K4_CONTAM_WORDS];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t min_l = trim + 1u;
  uint32_t n_hit = 0;  // (lane 0)
  for (uint32_t tile0 = 0; tile0 < cd.n; tile0 += K4_CONTAM_TILE) {
    const uint32_t nt = min((uint32_t)K4_CONTAM_TILE, cd.n - tile0);
    const bool last_tile = tile0 + nt == cd.n;
    __syncthreads();  // (the waves still reading the tile before)
    for (uint32_t i = tid; i < K4_CONTAM_ROWS * nt; i += K4_CONTAM_THREADS) {
      const uint32_t row = i / nt, e = i - row * nt;
      s_bits[row * K4_CONTAM_TILE + e] = cd.bits[(size_t)row * cd.n + tile0 + e];
    }
    for (uint32_t i = tid; i < nt; i += K4_CONTAM_THREADS) s_len[i] = cd.lens[tile0 + i];
    __syncthreads();
    for (uint32_t L = tid; L < (uint32_t)K4_CONTAM_MAX_LEN + 2u; L += K4_CONTAM_THREADS) {
      uint32_t lo = 0, hi = nt;  // the first entry shorter than L
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_len[mid] >= L) lo = mid + 1u; else hi = mid;
      }
      s_cnt[L] = (uint16_t)lo;
    }
    __syncthreads();
    const uint32_t longest = s_len[0];
    // G lanes share an overlap length, 64 / G lengths go in one step
    uint32_t G = 64u;
    while (G > 1u && (G >> 1) >= nt) G >>= 1;
    const uint32_t per_step = 64u / G, my_dl = lane / G, my_c = lane & (G - 1u);
    for (int64_t unit = (int64_t)blockIdx.x * (K4_CONTAM_THREADS / 64) + wave; unit < n_units;
         unit += (int64_t)gridDim.x * (K4_CONTAM_THREADS / 64)) {
      const bool sampled = sample_nth <= 1u || (uint64_t)(first_unit + unit) % sample_nth == 0u;
      const uint32_t rl = lens[unit];
      uint32_t best = 0;
      const uint32_t l_max = min(rl, longest);
      if (sampled && rl >= (uint32_t)K4_CONTAM_MIN_READ && rl <= (uint32_t)K4_CONTAM_MAX_READ && l_max >= min_l) {
        // the read end, packed by ballots: lane p of word w holds position 64 w + p
        const uint8_t* rd = reads + base + offs[unit];
        for (uint32_t w = 0; w < (uint32_t)K4_CONTAM_WORDS; w++) {
          const int64_t at = k4c_read_index(five != 0, rl, w * 64u + lane);
          const uint32_t planes = at >= 0 ? k4c_read_planes(rd[at]) : 0u;
          for (uint32_t pl = 0; pl < (uint32_t)K4_CONTAM_PLANES; pl++) {
            const uint64_t word = __ballot(planes >> pl & 1u);
            if (lane == 0u) s_read[wave][pl * 4u + w] = word;
          }
        }
        __builtin_amdgcn_wave_barrier();
        const LdsReadView rv{s_read[wave]};
        for (int l_top = (int)l_max; l_top >= (int)min_l && !best; l_top -= (int)per_step) {
          const int my_l = l_top - (int)my_dl;
          const uint32_t cnt = my_l >= (int)min_l ? s_cnt[my_l] : 0u;
          const uint32_t cnt_max = s_cnt[max(l_top - (int)per_step + 1, (int)min_l)];  // (the shortest length of the step has the most)
          bool acc = false;
          for (uint32_t c0 = 0; c0 < cnt_max; c0 += G) {
            const uint32_t c = c0 + my_c;
            if (c < cnt && !acc) acc = k4_contam_subs(rv, LdsContamView{s_bits, c}, (uint32_t)my_l, five != 0) <= 1u;
          }
          const uint64_t any = __ballot(acc);
          if (any) best = (uint32_t)l_top - (uint32_t)(__ffsll((unsigned long long)any) - 1) / G;  // lower lanes hold longer overlaps
        }
        __builtin_amdgcn_wave_barrier();  // (s_read is rewritten on the next trip)
      }
      if (lane == 0u) {
        uint32_t val = best > trim ? best - trim : 0u;
        uint8_t* o = out + unit * out_stride + out_ofs;
        if (tile0) val = max(val, (uint32_t)*o);
        *o = (uint8_t)val;
        if (last_tile && val) n_hit++;
      }
    }
  }
  if (lane == 0u && n_hit) atomicAdd(tot, (unsigned long long)n_hit);
}

}  // namespace

int k4i_contam_upload(k4_index* ix, const k4_contaminant* tbl, int32_t n, K4ContamDev* out) {
  if (!ix || !out || n < 0 || (n && !tbl) || n > K4_CONTAM_MAX_ENTRIES) return K4_ERR_PARAMS;
  K4_HIP(ix, hipSetDevice(ix->device));
  for (int cls = 0; cls < 4; cls++) {
    std::vector<const k4_contaminant*> es;
    for (int32_t k = 0; k < n; k++) {
      if (tbl[k].cls > 3 || tbl[k].len < K4_CONTAM_MIN_LEN || tbl[k].len > K4_CONTAM_MAX_LEN) return k4_fail(ix, K4_ERR_PARAMS, "contaminant %d: class %u, length %u", (int)k, tbl[k].cls, tbl[k].len);
      if (tbl[k].cls == cls) es.push_back(tbl + k);
    }
    std::stable_sort(es.begin(), es.end(), [](const k4_contaminant* a, const k4_contaminant* b) { return a->len > b->len; });
    const size_t m = es.size();
    out->n[cls] = (uint32_t)m;
    out->bits[cls].release();
    out->lens[cls].release();
    if (!m) continue;
    std::vector<uint64_t> rows((size_t)K4_CONTAM_ROWS * m);
    std::vector<uint16_t> ls(m);
    for (size_t e = 0; e < m; e++) {
      ls[e] = es[e]->len;
      for (int w = 0; w < 4; w++) {
        rows[(size_t)(0 + w) * m + e] = es[e]->p0[w];
        rows[(size_t)(4 + w) * m + e] = es[e]->p1[w];
        rows[(size_t)(8 + w) * m + e] = es[e]->nmask[w];
      }
    }
    K4_HIP(ix, out->bits[cls].alloc(rows.size() * 8));
    K4_HIP(ix, out->lens[cls].alloc(m * 2));
    K4_HIP(ix, hipMemcpy(out->bits[cls].p, rows.data(), rows.size() * 8, hipMemcpyHostToDevice));
    K4_HIP(ix, hipMemcpy(out->lens[cls].p, ls.data(), m * 2, hipMemcpyHostToDevice));
  }
  return K4_OK;
}

int k4i_contam_trims(k4_index* ix, const K4ContamDev& t, int pe, int64_t n, int32_t trim5, int32_t trim3, int32_t sample_nth,
                     int64_t first_unit, const void* d_reads, const void* d_offs1, const void* d_lens1, const void* d_offs2,
                     const void* d_lens2, uint64_t reads2_base, void* d_contam5, void* d_contam3, uint64_t* totals4, hipStream_t st) {
  if (!ix || n < 0 || trim5 < 0 || trim3 < 0 || trim5 > 50 || trim3 > 50 || sample_nth < 0 || first_unit < 0) return K4_ERR_PARAMS;
  if (totals4) totals4[0] = totals4[1] = totals4[2] = totals4[3] = 0;
  if (n == 0) return K4_OK;
  if (!d_reads || !d_offs1 || !d_lens1 || !d_contam5 || !d_contam3 || (pe && (!d_offs2 || !d_lens2))) return k4_fail(ix, K4_ERR_PARAMS, "null buffer");
  K4_HIP(ix, hipSetDevice(ix->device));
  const int64_t n_reads = pe ? 2 * n : n;
  K4PoolBuf tot;
  K4_HIP(ix, tot.alloc(32, st));
  K4_HIP(ix, hipMemsetAsync(tot.p, 0, 32, st));
  K4_HIP(ix, hipMemsetAsync(d_contam5, 0, (size_t)n_reads, st));  // (a class without entries trims nothing)
  K4_HIP(ix, hipMemsetAsync(d_contam3, 0, (size_t)n_reads, st));
  int cus = 0;
  K4_HIP(ix, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix->device));
  const unsigned blocks = (unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)std::max(cus, 1) * 4);  // four blocks of 39 KB LDS fit a CU
  for (int cls = 0; cls < (pe ? 4 : 3); cls++) {
    if ((!pe && cls == 1) || !t.n[cls]) continue;
    const bool five = cls < 2, second = (cls & 1) != 0;
    const ContamClassArg cd{t.bits[cls].as<uint64_t>(), t.lens[cls].as<uint16_t>(), t.n[cls]};
    hipLaunchKernelGGL(k4k_contam_trims, dim3(blocks), dim3(K4_CONTAM_THREADS), 0, st, cd, five ? 1 : 0, n, pe ? 2 : 1, second ? 1 : 0,
                       (uint32_t)(five ? trim5 : trim3), (uint32_t)sample_nth, first_unit, (const uint8_t*)d_reads,
                       (const uint64_t*)(second ? d_offs2 : d_offs1), (const uint32_t*)(second ? d_lens2 : d_lens1),
                       second ? reads2_base : (uint64_t)0, (uint8_t*)(five ? d_contam5 : d_contam3),
                       tot.as<unsigned long long>() + (second ? 2 : 0) + (five ? 0 : 1));
    K4_HIP(ix, hipGetLastError());
  }
  unsigned long long c[4];
  K4_HIP(ix, hipMemcpyAsync(c, tot.p, 32, hipMemcpyDeviceToHost, st));
  K4_HIP(ix, hipStreamSynchronize(st));
  if (totals4) for (int k = 0; k < 4; k++) totals4[k] = c[k];
  return K4_OK;
}

extern "C" int k4_contam_trims_dev(k4_index* ix, const k4_contaminant* tbl, int32_t n, int pe, int64_t n_units, int32_t trim5, int32_t trim3,
                                   int32_t sample_nth, int64_t first_unit, const void* d_reads, const void* d_offs1, const void* d_lens1,
                                   const void* d_offs2, const void* d_lens2, uint64_t reads2_base, void* d_contam5, void* d_contam3,
                                   uint64_t* totals4, void* stream) {
  if (!ix) return K4_ERR_PARAMS;
  K4ContamDev t;
  int rc = k4i_contam_upload(ix, tbl, n, &t);
  if (rc != K4_OK) return rc;
  // (waits for the stream: the table is let go of behind the kernels that read it)
  return k4i_contam_trims(ix, t, pe, n_units, trim5, trim3, sample_nth, first_unit, d_reads, d_offs1, d_lens1, d_offs2, d_lens2, reads2_base,
                          d_contam5, d_contam3, totals4, (hipStream_t)stream);
}
