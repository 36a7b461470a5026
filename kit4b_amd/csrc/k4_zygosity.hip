// kit4b_amd/csrc/k4_zygosity.hip -- `genzygosity` (genzygosity/genzygosity.cpp: ThreadedCoredApprox, :1122-1236) and the CSfxArray
// call under it, LocateAllNearMatches (libkit4b/SfxArray.cpp:4820-5091), on gfx950.  One WAVE per probe; the probe and its
// reverse complement sit in LDS.
//   k4z_near             the call for one probe: lane i resolves core i % n_core of strand i / n_core (k4q_count), then
//                          the unordered path: every run is walked 64 suffixes at a time, each lane extends its candidate, and a
//                            match counts when no earlier core window of the pass matches the target exactly at the same left end;
//                          the ordered path, when a run of a pass is longer than CurMaxIter or the runs of a pass reach the node
//                            limit: the lanes still extend 64 candidates at a time, lane 0 then takes them in suffix order through
//                            the dedupe set, IterCnt, the check at the 100th iteration, CurMaxIter, the node limit and MaxMatches.
//   k4z_near_matches     a batch of given probes; k4z_near_matches_big: those whose dedupe set outgrows LDS, with tables in HBM
//   k4z_zygosity_scan    one wave per start locus of a window of source entries; k4z_zygosity_scan_big likewise
//   k4z_zygosity_tally   the totals from the status bytes
// DESIGN.md "genzygosity: two walks, one answer" has the argument for the two paths and for the order-free matrix.
#include <algorithm>
#include "k4_stage.h"

#define K4Z_MAX_PROBE 1000      // cMaxSubseqLen, genzygosity.h:27
#define K4Z_MAX_CORES 32
#define K4Z_LAUNCH 16384        // probes (waves) per launch
#define K4Z_GROUP 64            // launches of the scan between two looks at the list of deferred windows
#define K4Z_REWALK 0x80000000u  // list entry of a given probe: its unordered walk has ended in -1, only the ordered one is left
#define K4Z_LDS_SLOTS 2048      // the dedupe table in LDS: the ids of a pass at half load, 1024
#define K4Z_MAX_ENTRIES 16384   // the per-wave bitmap of the scan
#define K4Z_BIG_BYTES (256u << 20)  // what the second launch's tables may take together

enum { K4Z_SKIP = -1, K4Z_REJECT = -2, K4Z_SELF = -3, K4Z_OWN = -4 };  // a candidate's fate; >= 0: the foreign entry it matched
enum { K4Z_DEFER = -2, K4Z_TABLE = -3 };                               // k4z_near beside -1 and the total
enum { K4Z_ST_ORDERED = 0x10, K4Z_ST_NO_WINDOW = 0x20 };               // internal bits of a status byte
enum { K4Z_CTL_LISTED = 0, K4Z_CTL_MAX_IDS = 1, K4Z_CTL_TABLE = 2, K4Z_CTL_TOTALS = 4 };  // 64-bit words of the control block

struct K4ZLimits { uint32_t max_tot_mm, core_len, core_delta, max_core_slides, max_matches, cur_max_iter, n_ident_nodes; };

struct K4ZShared {
  uint8_t pb[2][K4Z_MAX_PROBE];  // the probe as given, its reverse complement (low nibbles)
  uint32_t ofs[K4Z_MAX_CORES];
  uint32_t tid[64];
  int32_t out[64];
  uint32_t ctl[8];
  uint32_t table[K4Z_LDS_SLOTS];
  uint32_t seen[K4Z_MAX_ENTRIES / 32];
};

// where a foreign match is counted: the dense row of a given probe (may be null), the scan's bitmap (may be null)
struct K4ZSink {
  uint32_t* row;
  uint32_t* seen;
  K4_DEV void count(const K4DevIndex& ix, int e) const {
    const uint32_t id = ix.ent_id[e];  // pEntryMatches[EntryID - 1] while EntryID <= NumEntries (:5070)
    if (id < 1 || id > ix.n_entries) return;
    if (row) atomicAdd(&row[id - 1], 1u);
    if (seen) atomicOr(&seen[(id - 1) >> 5], 1u << ((id - 1) & 31));
  }
};

// the offsets of :4906-4917 while the node limit does not end the loop; every lane computes them
K4_DEV uint32_t k4z_core_offsets(const K4ZLimits& p, uint32_t len, uint32_t* ofs_out, int lane) {
  uint32_t n = 0, ofs = 0, delta = p.core_delta;
  while (n < p.max_core_slides && n < K4Z_MAX_CORES && ofs + p.core_len <= len && delta > p.core_len / 3) {
    if (ofs + p.core_len + delta > len) delta = len - (ofs + p.core_len);
    if (lane == 0) ofs_out[n] = ofs;
    n++;
    ofs += delta;
  }
  return n;
}

// the extension of :5024-5045 and the classification of :5048-5059 for the candidate whose left end is `left`; dirty gets a bit
// for every core window that holds a mismatch
K4_DEV int k4z_extend(const K4DevIndex& ix, K4Tb& tb, const K4ZLimits& p, const uint8_t* pbs, uint32_t len, const uint32_t* ofs, uint32_t n_core,
                      uint64_t left, uint32_t probe_id, uint32_t probe_ofs, uint32_t& dirty) {
  uint32_t mm = 0;
  dirty = 0;
  for (uint32_t j = 0; j < len; j++) {
    const uint32_t t = tb.get((int64_t)(left + j));
    if (t == 7u) return K4Z_REJECT;
    if (t == pbs[j]) continue;
    if (++mm > p.max_tot_mm) return K4Z_REJECT;
    for (uint32_t k = 0; k < n_core; k++)
      if (j >= ofs[k] && j < ofs[k] + p.core_len) dirty |= 1u << k;
  }
  const int e = k4d_map_entry(ix, left);
  if (e < 0) return K4Z_REJECT;
  if (ix.ent_id[e] != probe_id) return e;
  return (uint32_t)(left - ix.ent_start[e]) == probe_ofs ? K4Z_SELF : K4Z_OWN;
}

// the dedupe set of a pass: open addressing over 32-bit TargSeqIDs, 0 = free (the id 0 has a flag of its own)
K4_DEV bool k4z_insert(uint32_t* slots, uint32_t mask, uint32_t tid, bool& zero) {
  if (tid == 0) {
    const bool fresh = !zero;
    zero = true;
    return fresh;
  }
  uint32_t h = (tid * 2654435761u) & mask;
  while (slots[h]) {
    if (slots[h] == tid) return false;
    h = (h + 1) & mask;
  }
  slots[h] = tid;
  return true;
}

// LocateAllNearMatches for the probe in sh.pb.  Returns -1 or the total; K4Z_DEFER when the ordered path needs a table larger than
// LDS holds and `big` is null (*ids = the ids it has to hold); K4Z_TABLE when big is too small (cannot be: the host sizes it).
// ordered: the probe took the ordered path.  On -1 the row is as the sequential walk leaves it: a probe that ends in -1 on the
// unordered path with a row to fill is walked again in order (rewalk: that is all that is left of it; a deferred one says so).
template <int EL>
K4_DEV int k4z_near(const K4DevIndex& ix, K4Tb& tb, const K4ZLimits& p, K4ZShared& sh, uint32_t len, uint32_t probe_id, uint32_t probe_ofs,
                    const K4ZSink& sink, uint32_t* big, uint32_t big_slots, bool& ordered, uint32_t& ids, bool& rewalk) {
  const int lane = threadIdx.x;
  ordered = false;
  ids = 0;
  const uint32_t n_core = k4z_core_offsets(p, len, sh.ofs, lane);
  __syncthreads();
  // the runs, one per lane
  uint64_t first;
  const uint32_t cnt = k4d_cores_to_lanes<EL>(
      ix, tb, lane, 2 * n_core, n_core, p.core_len, 0xFFFFFFFFu, [&](uint32_t s) { return K4QSeq{sh.pb[s], len, 0}; },
      [&](uint32_t core) { return sh.ofs[core]; }, first);
  // which path: per pass the runs' sum against the node limit, the longest run against CurMaxIter; ids = what a pass can insert
  uint32_t pass_ids[2];
  for (uint32_t s = 0; s < 2; s++) {
    const bool mine = (uint32_t)lane >= s * n_core && (uint32_t)lane < (s + 1) * n_core;
    const uint64_t sum = k4d_wave_sum((uint64_t)(mine ? cnt : 0u));
    const uint64_t cap = k4d_wave_sum((uint64_t)(mine ? (p.cur_max_iter ? min(cnt, p.cur_max_iter) : cnt) : 0u));
    if (__ballot(mine && p.cur_max_iter && cnt > p.cur_max_iter) || sum >= p.n_ident_nodes) ordered = true;
    pass_ids[s] = (uint32_t)min(cap, (uint64_t)p.n_ident_nodes);
  }
  ids = max(pass_ids[0], pass_ids[1]);
  uint32_t total = 0;
  if (!ordered && !rewalk) {
    bool minus_one = false;
    for (uint32_t it = 0; it < 2 * n_core && !minus_one; it++) {
      const uint32_t k = it % n_core, ofs = sh.ofs[k];
      const uint8_t* pbs = sh.pb[it / n_core];
      k4d_run_walk<EL>(ix, lane, __shfl(first, (int)it, 64), __shfl(cnt, (int)it, 64), [&](uint32_t, uint64_t pos, bool active) {
        int out = K4Z_SKIP;
        if (active && pos >= ofs && pos - ofs + len <= ix.n) {
          uint32_t dirty;
          out = k4z_extend(ix, tb, p, pbs, len, sh.ofs, n_core, pos - ofs, probe_id, probe_ofs, dirty);
          if (~dirty & ((1u << k) - 1u)) out = K4Z_SKIP;  // an earlier core of this pass has met it
        }
        if (out >= 0) sink.count(ix, out);
        total += (uint32_t)__popcll(__ballot(out >= 0));
        minus_one = __ballot(out == K4Z_OWN) != 0 || (p.max_matches > 0 && total > p.max_matches);
        return minus_one;
      });
    }
    if (!minus_one) return (int)total;
    if (!sink.row) return -1;
    // the row of a -1 is what the walk had counted when it returned: take the probe through the ordered walk
    __threadfence();
    __syncthreads();
    for (uint32_t e = (uint32_t)lane; e < ix.n_entries; e += 64) sink.row[e] = 0;
    __threadfence();
    __syncthreads();
    total = 0;
    rewalk = true;
  }
  // the ordered walk
  uint32_t* slots = sh.table;
  if (ids > K4Z_LDS_SLOTS / 2) {
    if (!big) return K4Z_DEFER;
    slots = big;
  }
  for (uint32_t s = 0; s < 2; s++) {
    uint32_t n_slots = 64;
    while (n_slots < 2 * pass_ids[s]) n_slots <<= 1;
    if (n_slots > (slots == sh.table ? (uint32_t)K4Z_LDS_SLOTS : big_slots)) return K4Z_TABLE;
    __syncthreads();
    for (uint32_t i = (uint32_t)lane; i < n_slots; i += 64) slots[i] = 0;
    __threadfence_block();
    __syncthreads();
    const uint8_t* pbs = sh.pb[s];
    uint32_t nodes = 0;
    bool zero = false;
    for (uint32_t k = 0; k < n_core && nodes < p.n_ident_nodes; k++) {
      const uint32_t c = __shfl(cnt, (int)(s * n_core + k), 64);
      const uint32_t ofs = sh.ofs[k];
      uint32_t iter = 0;
      bool copies_known = false, stop = false, minus_one = false;
      k4d_run_walk<EL>(ix, lane, __shfl(first, (int)(s * n_core + k), 64), c, [&](uint32_t i0, uint64_t pos, bool active) {
        const uint32_t c0 = i0 - (uint32_t)lane;
        int out = K4Z_SKIP;
        uint32_t tid = 0;
        if (active && pos >= ofs && pos - ofs + len <= ix.n) {
          uint32_t dirty;
          tid = (uint32_t)(1 + pos - ofs);
          out = k4z_extend(ix, tb, p, pbs, len, sh.ofs, n_core, pos - ofs, probe_id, probe_ofs, dirty);
        }
        __syncthreads();  // (lane 0 has read the chunk before)
        sh.tid[lane] = tid;
        sh.out[lane] = out;
        __syncthreads();
        if (lane == 0) {
          const uint32_t m = min(64u, c - c0);
          int ret = 0;
          for (uint32_t j = 0; j < m && !stop && !ret; j++) {
            const uint32_t i = c0 + j;
            if ((p.cur_max_iter && iter >= p.cur_max_iter) || nodes >= p.n_ident_nodes) { stop = true; break; }
            if (i > 0 && iter == 100 && !copies_known) {  // :4938-4945: NumCopies = 1 + (index + 1 of the last) - (the element before)
              copies_known = true;
              if (p.cur_max_iter && c - i + 2 > p.cur_max_iter) { stop = true; break; }
            }
            const int o = sh.out[j];
            if (o == K4Z_SKIP || !k4z_insert(slots, n_slots - 1, sh.tid[j], zero)) continue;
            nodes++;
            iter++;
            if (o == K4Z_OWN) ret = 1;
            else if (o >= 0) {
              if (p.max_matches > 0 && total == p.max_matches) ret = 1;
              else { sink.count(ix, o); total++; }
            }
          }
          sh.ctl[0] = stop; sh.ctl[1] = (uint32_t)ret; sh.ctl[2] = iter; sh.ctl[3] = nodes; sh.ctl[4] = total; sh.ctl[5] = copies_known; sh.ctl[6] = zero;
        }
        __syncthreads();
        stop = sh.ctl[0] != 0; iter = sh.ctl[2]; nodes = sh.ctl[3]; total = sh.ctl[4]; copies_known = sh.ctl[5] != 0; zero = sh.ctl[6] != 0;
        minus_one = sh.ctl[1] != 0;
        return stop || minus_one;
      });
      if (minus_one) return -1;
    }
  }
  return (int)total;
}

struct K4ZNearArgs {
  K4DevIndex ix;
  K4ZLimits p;
  int64_t n;
  const uint8_t* seqs;
  const uint64_t* offs;
  const uint32_t* lens;
  const uint32_t* probe_entries;
  const uint32_t* probe_ofs;
  int32_t* rslt;
  uint32_t* counts;     // n x n_entries, or null
  uint32_t* list;       // the probes that wait for the second launch
  unsigned long long* ctl;
  uint32_t* big;        // second launch: big_slots words per block
  uint32_t big_slots;
};

template <int EL>
K4_DEV void k4z_one_probe(const K4ZNearArgs& a, K4ZShared& sh, K4Tb& tb, int64_t i, bool second, bool rewalk) {
  const int lane = threadIdx.x;
  const uint32_t len = a.lens[i];
  __syncthreads();  // (the probe before has been read)
  for (uint32_t j = (uint32_t)lane; j < len; j += 64) {
    const uint32_t b = a.seqs[a.offs[i] + j] & 0x0fu;
    sh.pb[0][j] = (uint8_t)b;
    sh.pb[1][len - 1 - j] = (uint8_t)(b <= 3 ? 3 - b : b);
  }
  uint32_t* row = a.counts ? a.counts + (uint64_t)i * a.ix.n_entries : nullptr;
  if (row && !second)
    for (uint32_t e = (uint32_t)lane; e < a.ix.n_entries; e += 64) row[e] = 0;
  __threadfence();
  __syncthreads();
  K4ZLimits p = a.p;
  if (p.core_len > len) p.core_len = len;  // (refused on the host; keeps every index inside the probe)
  const K4ZSink sink = {row, nullptr};
  bool ordered;
  uint32_t ids;
  const int r = k4z_near<EL>(a.ix, tb, p, sh, len, a.probe_entries[i], a.probe_ofs[i], sink, second ? a.big + (uint64_t)blockIdx.x * a.big_slots : nullptr,
                             a.big_slots, ordered, ids, rewalk);
  if (lane != 0) return;
  if (r == K4Z_DEFER) {
    a.list[atomicAdd(&a.ctl[K4Z_CTL_LISTED], 1ull)] = (uint32_t)i | (rewalk ? K4Z_REWALK : 0u);
    atomicMax(&a.ctl[K4Z_CTL_MAX_IDS], (unsigned long long)ids);
  } else if (r == K4Z_TABLE) {
    atomicAdd(&a.ctl[K4Z_CTL_TABLE], 1ull);
  } else {
    a.rslt[i] = r;
  }
}

template <int EL>
__global__ void __launch_bounds__(64) k4z_near_matches(K4ZNearArgs a) {
  __shared__ K4ZShared sh;
  K4Tb tb;
  tb.init(a.ix);
  for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) k4z_one_probe<EL>(a, sh, tb, i, false, false);
}

template <int EL>
__global__ void __launch_bounds__(64) k4z_near_matches_big(K4ZNearArgs a, uint32_t n_listed) {
  __shared__ K4ZShared sh;
  K4Tb tb;
  tb.init(a.ix);
  for (uint32_t q = blockIdx.x; q < n_listed; q += gridDim.x) k4z_one_probe<EL>(a, sh, tb, (int64_t)(a.list[q] & ~K4Z_REWALK), true, (a.list[q] & K4Z_REWALK) != 0);
}

struct K4ZScanArgs {
  K4DevIndex ix;
  K4ZLimits p;
  const uint64_t* pre;   // src_count + 1: start loci of the source entries in front
  uint32_t src_first;    // ordinal (0-based) of the first source entry
  uint32_t src_count;
  uint32_t subseq_len, max_ns;
  uint64_t k0, k1;       // this launch's start loci
  uint64_t g0;           // the first start locus of this group of launches: the list holds offsets from it
  uint32_t* matrix;      // src_count x n_entries
  uint32_t* subseqs;
  uint8_t* status;       // internal: with the K4Z_ST_* bits
  uint32_t* list;
  unsigned long long* ctl;
  uint32_t* big;
  uint32_t big_slots;
};

template <int EL>
K4_DEV void k4z_one_locus(const K4ZScanArgs& a, K4ZShared& sh, K4Tb& tb, uint64_t pid, bool second) {
  const int lane = threadIdx.x;
  const uint32_t r = k4d_last_le(a.src_count, pid, [&](uint32_t i) { return a.pre[i]; });  // the source entry that holds start locus pid
  const uint32_t e = a.src_first + r, locus = (uint32_t)(pid - a.pre[r]), len = a.subseq_len;
  const uint32_t seq_len = (uint32_t)(a.ix.ent_end[e] - a.ix.ent_start[e] + 1);
  if (seq_len < len || locus > seq_len - len) {
    if (lane == 0) a.status[pid] = K4Z_ST_NO_WINDOW;
    return;
  }
  const uint64_t cpos = a.ix.ent_start[e] + locus;
  __syncthreads();  // (the locus before has been read)
  uint32_t ns = 0;
  bool bad = false;
  for (uint32_t j = (uint32_t)lane; j < len; j += 64) {  // :1171-1186
    const uint32_t b = tb.get((int64_t)(cpos + j)) & 0x07u;
    sh.pb[0][j] = (uint8_t)b;
    sh.pb[1][len - 1 - j] = (uint8_t)(b <= 3 ? 3 - b : b);
    bad |= b > 4u;
    ns += b == 4u;
  }
  const uint32_t words = (a.ix.n_entries + 31) >> 5;
  for (uint32_t w = (uint32_t)lane; w < words; w += 64) sh.seen[w] = 0;
  ns = k4d_wave_sum(ns);
  const bool over = __ballot(bad) != 0 || ns > a.max_ns;
  __syncthreads();
  if (over) {
    if (lane == 0) a.status[pid] = 0;
    return;
  }
  const K4ZSink sink = {nullptr, sh.seen};
  bool ordered, rewalk = false;  // (no row: a -1 of the unordered walk is final)
  uint32_t ids;
  const int rs = k4z_near<EL>(a.ix, tb, a.p, sh, len, a.ix.ent_id[e], locus, sink, second ? a.big + (uint64_t)blockIdx.x * a.big_slots : nullptr,
                              a.big_slots, ordered, ids, rewalk);
  if (rs == K4Z_DEFER || rs == K4Z_TABLE) {
    if (lane == 0) {
      if (rs == K4Z_DEFER) {
        a.list[atomicAdd(&a.ctl[K4Z_CTL_LISTED], 1ull)] = (uint32_t)(pid - a.g0);
        atomicMax(&a.ctl[K4Z_CTL_MAX_IDS], (unsigned long long)ids);
      } else {
        atomicAdd(&a.ctl[K4Z_CTL_TABLE], 1ull);
      }
    }
    return;
  }
  const uint8_t flag = ordered ? K4Z_ST_ORDERED : 0;
  if (rs < 0) {
    if (lane == 0) a.status[pid] = 1 | flag;
    return;
  }
  __syncthreads();  // (the marks of every lane are in the bitmap)
  if (rs > 0) {     // :1212-1222: one for every entry the window hit
    for (uint32_t w = (uint32_t)lane; w < words; w += 64) {
      uint32_t bits = sh.seen[w];
      while (bits) {
        const uint32_t b = (uint32_t)__ffs(bits) - 1u;
        bits &= bits - 1u;
        atomicAdd(&a.matrix[(uint64_t)r * a.ix.n_entries + w * 32 + b], 1u);
      }
    }
  }
  if (lane == 0) {
    atomicAdd(&a.subseqs[r], 1u);
    a.status[pid] = (rs > 0 ? 3 : 2) | flag;
  }
}

template <int EL>
__global__ void __launch_bounds__(64) k4z_zygosity_scan(K4ZScanArgs a) {
  __shared__ K4ZShared sh;
  const uint64_t pid = a.k0 + blockIdx.x;
  if (pid >= a.k1) return;
  K4Tb tb;
  tb.init(a.ix);
  k4z_one_locus<EL>(a, sh, tb, pid, false);
}

template <int EL>
__global__ void __launch_bounds__(64) k4z_zygosity_scan_big(K4ZScanArgs a, uint32_t n_listed) {
  __shared__ K4ZShared sh;
  K4Tb tb;
  tb.init(a.ix);
  for (uint32_t q = blockIdx.x; q < n_listed; q += gridDim.x) k4z_one_locus<EL>(a, sh, tb, a.g0 + a.list[q], true);
}

// windows, passed over, rejected, unique, unique with matches, ordered from the internal status bytes; the caller's bytes are
// those without the internal bits
__global__ void __launch_bounds__(256) k4z_zygosity_tally(const uint8_t* status, uint64_t n, uint8_t* user, unsigned long long* tot) {
  uint32_t c[6] = {0, 0, 0, 0, 0, 0};
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) {
    const uint32_t s = status[p];
    if (user) user[p] = (uint8_t)(s & 3u);
    if (s & K4Z_ST_NO_WINDOW) continue;
    c[0]++;
    c[1] += (s & 3u) == 0;
    c[2] += (s & 3u) == 1;
    c[3] += (s & 3u) >= 2;
    c[4] += (s & 3u) == 3;
    c[5] += (s & K4Z_ST_ORDERED) != 0;
  }
  k4d_tally_flush(c, tot);
}

// ==== host side ======================================================================================================
// the second launch's tables: slots per block (a power of two that holds max_ids at half load) and how many blocks share
// K4Z_BIG_BYTES; the workspace only grows
static int zygosity_big(k4_index* ix, uint64_t max_ids, uint64_t n_listed, uint32_t* slots, unsigned* grid) {
  uint64_t s = 64;
  while (s < 2 * max_ids) s <<= 1;
  if (s > (1ull << 31)) return k4_fail(ix, K4_ERR_UNSUPPORTED, "LocateAllNearMatches: a dedupe set of %llu ids", (unsigned long long)max_ids);
  const uint64_t fit = std::max<uint64_t>(1, K4Z_BIG_BYTES / (s * 4));
  *grid = (unsigned)std::min<uint64_t>(std::min<uint64_t>(n_listed, fit), K4Z_LAUNCH);
  *slots = (uint32_t)s;
  K4_HIP(ix, ix->zyg.big.reserve((size_t)(*grid * s * 4)));
  return K4_OK;
}

static int check_limits(k4_index* ix, const k4_near_params* p, K4ZLimits* l) {
  if (p->core_len < 1 || p->core_delta < 1 || p->max_core_slides < 1 || p->max_core_slides > K4Z_MAX_CORES)
    return k4_fail(ix, K4_ERR_PARAMS, "LocateAllNearMatches: core_len %d or core_delta %d below 1, or max_core_slides %d outside 1..%d", p->core_len,
                   p->core_delta, p->max_core_slides, K4Z_MAX_CORES);
  if (p->max_tot_mm < 0 || p->max_matches < 0 || p->cur_max_iter < 0 || p->n_ident_nodes < 0)
    return k4_fail(ix, K4_ERR_PARAMS, "LocateAllNearMatches: a limit below 0 (max_tot_mm %d, max_matches %d, cur_max_iter %d, n_ident_nodes %d)", p->max_tot_mm,
                   p->max_matches, p->cur_max_iter, p->n_ident_nodes);
  l->max_tot_mm = (uint32_t)p->max_tot_mm; l->core_len = (uint32_t)p->core_len; l->core_delta = (uint32_t)p->core_delta;
  l->max_core_slides = (uint32_t)p->max_core_slides; l->max_matches = (uint32_t)p->max_matches; l->cur_max_iter = (uint32_t)p->cur_max_iter;
  l->n_ident_nodes = (uint32_t)p->n_ident_nodes;
  return K4_OK;
}

// the batch on device arrays, its arguments checked; ends with the stream waited for
static int near_run(k4_index* ix, const K4ZLimits& l, int64_t n, const uint8_t* d_seqs, const uint64_t* d_offs, const uint32_t* d_lens,
                    const uint32_t* d_entries, const uint32_t* d_ofs, int32_t* d_rslt, uint32_t* d_counts, hipStream_t st) {
  K4ZygState& z = ix->zyg;
  K4_HIP(ix, z.ctl.reserve(16 * 8));
  K4_HIP(ix, z.list.reserve((size_t)n * 4 + 16));
  K4_HIP(ix, hipMemsetAsync(z.ctl.p, 0, 16 * 8, st));
  K4ZNearArgs a;
  a.ix = ix->d; a.p = l; a.n = n; a.seqs = d_seqs; a.offs = d_offs; a.lens = d_lens; a.probe_entries = d_entries; a.probe_ofs = d_ofs;
  a.rslt = d_rslt; a.counts = d_counts; a.list = z.list.as<uint32_t>(); a.ctl = z.ctl.as<unsigned long long>(); a.big = nullptr; a.big_slots = 0;
  K4_HIP(ix, z.timer.begin(st));
  K4S_LAUNCH_EL(ix, k4z_near_matches, (unsigned)std::min<int64_t>(n, K4Z_LAUNCH), 64, st, a);
  K4_HIP(ix, hipGetLastError());
  unsigned long long c[3] = {0, 0, 0};
  K4_HIP(ix, hipMemcpyAsync(c, z.ctl.p, sizeof(c), hipMemcpyDeviceToHost, st));
  K4_HIP(ix, hipStreamSynchronize(st));
  z.second = c[K4Z_CTL_LISTED];
  if (c[K4Z_CTL_LISTED]) {
    unsigned grid = 0;
    K4_TRY(zygosity_big(ix, c[K4Z_CTL_MAX_IDS], c[K4Z_CTL_LISTED], &a.big_slots, &grid));
    a.big = z.big.as<uint32_t>();
    K4S_LAUNCH_EL(ix, k4z_near_matches_big, grid, 64, st, a, (uint32_t)c[K4Z_CTL_LISTED]);
    K4_HIP(ix, hipGetLastError());
    K4_HIP(ix, hipMemcpyAsync(c, z.ctl.p, sizeof(c), hipMemcpyDeviceToHost, st));
  }
  K4_HIP(ix, z.timer.end(st));
  K4_TRY(k4s_call_close(ix, st, z.timer));
  if (c[K4Z_CTL_TABLE]) return k4_fail(ix, K4_ERR_MEM, "LocateAllNearMatches: %llu probes outgrew their dedupe table", c[K4Z_CTL_TABLE]);
  return K4_OK;
}

static int near_check(k4_index* ix, const k4_near_params* p, int64_t n, const void* seqs, const void* offs, const void* lens, const void* entries,
                      const void* ofs, const void* rslts, const void* counts, uint64_t counts_cap, K4ZLimits* l) {
  if (!ix) return K4_ERR_PARAMS;
  ix->zyg.timer.reset();
  ix->zyg.second = 0;
  if (!p || n < 0 || n >= (int64_t)K4Z_REWALK || (n > 0 && (!seqs || !offs || !lens || !entries || !ofs || !rslts))) return k4_fail(ix, K4_ERR_PARAMS, "LocateAllNearMatches: null argument");
  K4_TRY(check_limits(ix, p, l));
  if (counts && counts_cap < (uint64_t)n * ix->d.n_entries)
    return k4_fail(ix, K4_ERR_PARAMS, "LocateAllNearMatches: room for %llu counts, %lld probes x %u entries", (unsigned long long)counts_cap, (long long)n,
                   ix->d.n_entries);
  return K4_OK;
}

static int near_check_lens(k4_index* ix, const K4ZLimits& l, int64_t n, const uint32_t* lens) {
  for (int64_t i = 0; i < n; i++)
    if (lens[i] > K4Z_MAX_PROBE || l.core_len > lens[i])
      return k4_fail(ix, K4_ERR_PARAMS, "LocateAllNearMatches: probe %lld of %u bases, at most %d and at least core_len %u", (long long)i, lens[i], K4Z_MAX_PROBE,
                     l.core_len);
  return K4_OK;
}

extern "C" int k4_all_near_matches_batch_dev(k4_index* ix, const k4_near_params* p, int64_t n, const void* d_seqs, const void* d_offs, const void* d_lens,
                                             const void* d_probe_entries, const void* d_probe_ofs, void* d_rslts, void* d_counts, uint64_t counts_cap,
                                             void* stream) {
  K4ZLimits l;
  K4_TRY(near_check(ix, p, n, d_seqs, d_offs, d_lens, d_probe_entries, d_probe_ofs, d_rslts, d_counts, counts_cap, &l));
  if (n == 0) return K4_OK;
  K4_HIP(ix, hipSetDevice(ix->device));
  const hipStream_t st = (hipStream_t)stream;
  std::vector<uint32_t> h_lens((size_t)n);  // (the length limits are checked on the host)
  K4_HIP(ix, hipMemcpyAsync(h_lens.data(), d_lens, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  K4_HIP(ix, hipStreamSynchronize(st));
  K4_TRY(near_check_lens(ix, l, n, h_lens.data()));
  return near_run(ix, l, n, (const uint8_t*)d_seqs, (const uint64_t*)d_offs, (const uint32_t*)d_lens, (const uint32_t*)d_probe_entries,
                  (const uint32_t*)d_probe_ofs, (int32_t*)d_rslts, (uint32_t*)d_counts, st);
}

extern "C" int k4_all_near_matches_batch(k4_index* ix, const k4_near_params* p, int64_t n, const uint8_t* seqs, const uint64_t* offs, const uint32_t* lens,
                                         const uint32_t* probe_entries, const uint32_t* probe_ofs, int32_t* rslts, uint32_t* counts, uint64_t counts_cap) {
  K4ZLimits l;
  K4_TRY(near_check(ix, p, n, seqs, offs, lens, probe_entries, probe_ofs, rslts, counts, counts_cap, &l));
  K4_TRY(near_check_lens(ix, l, n, lens));
  if (n == 0) return K4_OK;
  K4ZygState& z = ix->zyg;
  hipStream_t st;
  K4_TRY(k4s_call_open(ix, &st));
  K4_TRY(k4s_stage_seqs(ix, n, seqs, offs, lens, nullptr));
  const size_t n_counts = counts ? (size_t)n * ix->d.n_entries : 0;
  K4_HIP(ix, z.out.reserve((size_t)n * 12 + n_counts * 4 + 16));
  uint32_t* d_entries = z.out.as<uint32_t>();
  uint32_t* d_ofs = d_entries + n;
  int32_t* d_rslt = (int32_t*)(d_ofs + n);
  uint32_t* d_counts = counts ? (uint32_t*)(d_rslt + n) : nullptr;
  K4_HIP(ix, hipMemcpyAsync(d_entries, probe_entries, (size_t)n * 4, hipMemcpyHostToDevice, st));
  K4_HIP(ix, hipMemcpyAsync(d_ofs, probe_ofs, (size_t)n * 4, hipMemcpyHostToDevice, st));
  K4_TRY(near_run(ix, l, n, ix->seq_stage.seqs.as<uint8_t>(), ix->seq_stage.offs.as<uint64_t>(), ix->seq_stage.lens.as<uint32_t>(), d_entries, d_ofs,
                  d_rslt, d_counts, st));
  K4_HIP(ix, hipMemcpyAsync(rslts, d_rslt, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (counts) K4_HIP(ix, hipMemcpyAsync(counts, d_counts, n_counts * 4, hipMemcpyDeviceToHost, st));
  return k4s_call_close(ix, st, z.timer);
}

// the front end's derivation (genzygosity.cpp:681-697, :998-1027, :1190) from the scan's parameters and the index
static int zygosity_limits(k4_index* ix, const k4_zygosity_params* p, K4ZLimits* l) {
  if (p->subseq_len < 20 || p->subseq_len > K4Z_MAX_PROBE) return k4_fail(ix, K4_ERR_PARAMS, "genzygosity: subseq_len %d outside 20..%d", p->subseq_len, K4Z_MAX_PROBE);
  if (p->max_subs < 0 || p->max_subs > std::min(30, p->subseq_len - 18))
    return k4_fail(ix, K4_ERR_PARAMS, "genzygosity: max_subs %d outside 0..%d", p->max_subs, std::min(30, p->subseq_len - 18));
  if (p->max_ns < 0 || p->max_ns > 5) return k4_fail(ix, K4_ERR_PARAMS, "genzygosity: max_ns %d outside 0..5", p->max_ns);
  if (p->max_matches < 0 || p->max_matches > 1000000) return k4_fail(ix, K4_ERR_PARAMS, "genzygosity: max_matches %d outside 0..1000000", p->max_matches);
  if (p->mode < 0 || p->mode > 3) return k4_fail(ix, K4_ERR_PARAMS, "genzygosity: mode %d outside 0..3", p->mode);
  static const int add[4] = {4, 2, 0, 6}, slides[4] = {4, 6, 8, 3}, iters[4] = {5000, 25000, 50000, 1000};
  const int min_core = (ix->tot_seqs_len < 20000000 ? 5 : ix->tot_seqs_len < 250000000 ? 8 : 10) + add[p->mode];
  l->max_tot_mm = (uint32_t)p->max_subs;
  l->core_len = (uint32_t)std::min(p->subseq_len, std::max(min_core, p->subseq_len / (p->max_subs + 1)));
  l->core_delta = l->core_len;
  l->max_core_slides = (uint32_t)slides[p->mode];
  l->max_matches = (uint32_t)p->max_matches;
  l->cur_max_iter = (uint32_t)iters[p->mode];
  l->n_ident_nodes = K4_MAX_IDENT_NODES;
  return K4_OK;
}

// the scan; matrix, subseqs and status are device pointers here (on_host: those of z.out, brought down by the caller)
static int zygosity_run(k4_index* ix, const k4_zygosity_params* p, int32_t src_first, int32_t src_count, uint32_t* d_matrix, uint32_t* d_subseqs,
                        uint8_t* d_status, uint64_t status_len, bool on_host, k4_zygosity_totals* tot, uint64_t* total, hipStream_t st) {
  if (!ix) return K4_ERR_PARAMS;
  K4ZygState& z = ix->zyg;
  z.timer.reset();
  z.second = 0;
  if (!p || !tot || !d_matrix || !d_subseqs) return k4_fail(ix, K4_ERR_PARAMS, "genzygosity: null argument");
  K4ZLimits l;
  K4_TRY(zygosity_limits(ix, p, &l));
  const uint32_t n_ent = ix->d.n_entries;
  if (src_first < 1 || (uint32_t)src_first > n_ent || src_count < 0 || (uint64_t)src_first + (uint64_t)src_count - 1 > n_ent)
    return k4_fail(ix, K4_ERR_PARAMS, "genzygosity: source entries %d .. %d outside 1..%u", src_first, src_first + src_count - 1, n_ent);
  if (n_ent > K4Z_MAX_ENTRIES) return k4_fail(ix, K4_ERR_UNSUPPORTED, "genzygosity: %u entries, at most %d (the per-wave bitmap)", n_ent, K4Z_MAX_ENTRIES);
  std::vector<uint64_t> pre((size_t)src_count + 1, 0);
  for (int32_t r = 0; r < src_count; r++) pre[(size_t)r + 1] = pre[(size_t)r] + ix->entries[(size_t)(src_first - 1 + r)].seq_len;
  *total = pre[(size_t)src_count];
  if (d_status && status_len < *total)
    return k4_fail(ix, K4_ERR_PARAMS, "genzygosity: %llu status bytes, the source entries have %llu loci", (unsigned long long)status_len, (unsigned long long)*total);
  memset(tot, 0, sizeof(*tot));
  K4_HIP(ix, hipSetDevice(ix->device));
  const size_t m_bytes = (size_t)src_count * n_ent * 4, s_bytes = (size_t)src_count * 4;
  if (on_host) {  // matrix | subseqs | status
    K4_HIP(ix, z.out.reserve(m_bytes + s_bytes + (size_t)*total + 16));
    d_matrix = z.out.as<uint32_t>();
    d_subseqs = d_matrix + (size_t)src_count * n_ent;
    d_status = d_status ? (uint8_t*)(d_subseqs + src_count) : nullptr;
  }
  if (src_count > 0) {
    K4_HIP(ix, hipMemsetAsync(d_matrix, 0, m_bytes, st));
    K4_HIP(ix, hipMemsetAsync(d_subseqs, 0, s_bytes, st));
  }
  if (*total == 0) {
    K4_HIP(ix, hipStreamSynchronize(st));
    return K4_OK;
  }
  K4_HIP(ix, hipStreamSynchronize(st));  // (tables about to be replaced may still be read by the call before)
  K4_HIP(ix, z.pre.reserve(pre.size() * 8));
  K4_HIP(ix, z.status.reserve((size_t)*total + 16));
  K4_HIP(ix, z.list.reserve((size_t)std::min<uint64_t>(*total, (uint64_t)K4Z_GROUP * K4Z_LAUNCH) * 4 + 16));
  K4_HIP(ix, z.ctl.reserve(16 * 8));
  K4_HIP(ix, hipMemcpyAsync(z.pre.p, pre.data(), pre.size() * 8, hipMemcpyHostToDevice, st));
  K4_HIP(ix, hipMemsetAsync(z.ctl.p, 0, 16 * 8, st));
  unsigned long long* d_ctl = z.ctl.as<unsigned long long>();
  K4ZScanArgs a;
  a.ix = ix->d; a.p = l; a.pre = z.pre.as<uint64_t>(); a.src_first = (uint32_t)src_first - 1; a.src_count = (uint32_t)src_count;
  a.subseq_len = (uint32_t)p->subseq_len; a.max_ns = (uint32_t)p->max_ns; a.matrix = d_matrix; a.subseqs = d_subseqs; a.status = z.status.as<uint8_t>();
  a.list = z.list.as<uint32_t>(); a.ctl = d_ctl; a.big = nullptr; a.big_slots = 0;
  K4_HIP(ix, z.timer.begin(st));
  unsigned long long tables = 0;
  for (uint64_t g0 = 0; g0 < *total; g0 += (uint64_t)K4Z_GROUP * K4Z_LAUNCH) {
    const uint64_t g1 = std::min<uint64_t>(*total, g0 + (uint64_t)K4Z_GROUP * K4Z_LAUNCH);
    a.g0 = g0;
    a.big = nullptr;
    k4s_launch_windows(g1 - g0, K4Z_LAUNCH, [&](uint64_t k0, uint64_t k1) {
      a.k0 = g0 + k0;
      a.k1 = g0 + k1;
      K4S_LAUNCH_EL(ix, k4z_zygosity_scan, (unsigned)(k1 - k0), 64, st, a);
    });
    K4_HIP(ix, hipGetLastError());
    unsigned long long c[3] = {0, 0, 0};  // the windows of this group that wait for tables in HBM
    K4_HIP(ix, hipMemcpyAsync(c, d_ctl, sizeof(c), hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipStreamSynchronize(st));
    if (c[K4Z_CTL_LISTED]) {
      unsigned grid = 0;
      K4_TRY(zygosity_big(ix, c[K4Z_CTL_MAX_IDS], c[K4Z_CTL_LISTED], &a.big_slots, &grid));
      a.big = z.big.as<uint32_t>();
      K4S_LAUNCH_EL(ix, k4z_zygosity_scan_big, grid, 64, st, a, (uint32_t)c[K4Z_CTL_LISTED]);
      K4_HIP(ix, hipGetLastError());
      z.second += c[K4Z_CTL_LISTED];
      K4_HIP(ix, hipMemsetAsync(d_ctl, 0, 2 * 8, st));
    }
    tables += c[K4Z_CTL_TABLE];
  }
  hipLaunchKernelGGL(k4z_zygosity_tally, dim3((unsigned)std::min<uint64_t>((*total + 255) / 256, 1024)), dim3(256), 0, st, z.status.as<uint8_t>(), *total, d_status,
                     d_ctl + K4Z_CTL_TOTALS);
  K4_HIP(ix, hipGetLastError());
  K4_HIP(ix, z.timer.end(st));
  unsigned long long t16[16] = {0};
  K4_HIP(ix, hipMemcpyAsync(t16, d_ctl, sizeof(t16), hipMemcpyDeviceToHost, st));
  K4_TRY(k4s_call_close(ix, st, z.timer));
  if (tables || t16[K4Z_CTL_TABLE]) return k4_fail(ix, K4_ERR_MEM, "genzygosity: a window outgrew its dedupe table");
  const unsigned long long* t = t16 + K4Z_CTL_TOTALS;
  tot->windows = t[0]; tot->passed_over = t[1]; tot->rejected = t[2]; tot->unique = t[3]; tot->unique_matched = t[4]; tot->ordered = t[5];
  tot->second_launch = z.second;
  return K4_OK;
}

extern "C" int k4_zygosity_batch_dev(k4_index* ix, const k4_zygosity_params* p, int32_t src_first, int32_t src_count, void* d_matrix, void* d_subseqs,
                                     void* d_status, uint64_t status_len, k4_zygosity_totals* totals, void* stream) {
  uint64_t total = 0;
  return zygosity_run(ix, p, src_first, src_count, (uint32_t*)d_matrix, (uint32_t*)d_subseqs, (uint8_t*)d_status, status_len, false, totals, &total,
                      (hipStream_t)stream);
}

// host arrays: the matrix and subseqs are written whole; of status the bytes of the source entries' loci, the rest stays
extern "C" int k4_zygosity_batch(k4_index* ix, const k4_zygosity_params* p, int32_t src_first, int32_t src_count, uint32_t* matrix, uint32_t* subseqs,
                                 uint8_t* status, uint64_t status_len, k4_zygosity_totals* totals) {
  if (!ix) return K4_ERR_PARAMS;
  uint64_t total = 0;
  hipStream_t st;
  K4_TRY(k4s_call_open(ix, &st));
  const int rc = zygosity_run(ix, p, src_first, src_count, matrix, subseqs, status, status_len, true, totals, &total, st);
  if (rc != K4_OK || src_count == 0) return rc;
  K4ZygState& z = ix->zyg;
  const size_t cells = (size_t)src_count * ix->d.n_entries;
  K4_HIP(ix, hipMemcpyAsync(matrix, z.out.p, cells * 4, hipMemcpyDeviceToHost, st));
  K4_HIP(ix, hipMemcpyAsync(subseqs, z.out.as<uint32_t>() + cells, (size_t)src_count * 4, hipMemcpyDeviceToHost, st));
  if (status && total) K4_HIP(ix, hipMemcpyAsync(status, z.out.as<uint32_t>() + cells + src_count, (size_t)total, hipMemcpyDeviceToHost, st));
  return k4s_call_close(ix, st, z.timer);
}

extern "C" double k4_zygosity_last_kernel_ms(const k4_index* ix) { return ix ? ix->zyg.timer.ms : 0.0; }
