// kit4b_amd/csrc/k4_cults.hip -- CSfxArray::GenKMerCultsCnts with AntisenseKMerCultsCnts (libkit4b/SfxArray.cpp:2804-3133,
// `ngskit4b kmermarkers`) on gfx950, MaxHomozygotic == 0.  The reference walks the suffix array in order; here the walk is restated
// per element (DESIGN.md "K-mer cultivar counts"): with P = prefix_len, K = P + suffix_len, psn = SA[i]
//   X(i)  psn + K >= ConcatSeqLen          F(i)  not X and the K bases are ACGT
//   b(i)  i is the call's first element, or X(i), or the P bases at SA[i] differ from those at SA[i - 1]
// and the elements from one b to the next are a segment: one located K-mer when it holds an F element.  The range goes through in
// windows of at most max_window elements.  k4k_cult_flags writes b, F and the entry of every element of a window; rocPRIM selects the
// segment starts; k4k_cult_segments, one wave per segment, counts the F elements per entry into a histogram (LDS up to
// K4C_LDS_ENTRIES entries, a slice of global memory per block above), walks the run of the prefix's reverse complement over the
// whole index for the antisense side, and reads the histogram out in entry order.  It runs twice: a count pass gives every segment
// its place in the outputs (scans), a fill pass writes the records.  A window ends with the last segment that ends inside it; a
// segment longer than a window is taken alone, its end looked for window by window, and its wave tests the elements itself.
#include <algorithm>
#include "k4_stage.h"

#define K4C_DEFAULT_WINDOW (1u << 20)
#define K4C_MAX_WINDOW (1u << 24)
#define K4C_MIN_CAP_WINDOW 4096u  // a window is cut down to the room left in the outputs, but no further than this
#define K4C_MAX_KMERS (1ull << 21)  // one call writes no more K-mers / counts than this, whatever the caps: they bound the
#define K4C_MAX_DIST (1ull << 25)   // host-pointer form's staging (at most 32 + 300 bytes per K-mer and 12 per count)
#define K4C_LDS_ENTRIES 2048     // per-wave histogram in LDS up to here (16 KB); above: K4C_GLOBAL_BLOCKS slices of global memory
#define K4C_LDS_BLOCKS 2048
#define K4C_GLOBAL_BLOCKS 256
#define K4C_MAX_CULTIVARS 20000  // cMaxCultivars, SfxArray.h:186
#define K4C_NONE 0xFFFFFFFFFFFFFFFFull

struct K4CultFlagArgs {
  K4DevIndex ix;
  uint64_t w0, w1;   // the window's elements [w0, w1)
  uint64_t forced;   // the element that starts a segment whatever stands in front of it (the call's first), or K4C_NONE
  uint32_t P, K;
  uint8_t* flags;    // per element of the window: bit 0 = b, bit 1 = F
  uint32_t* ent;     // ... and the place of its entry in the entry table (F elements only)
};

struct K4CultSegArgs {
  K4DevIndex ix;
  const uint32_t* seg_start;  // window-relative first elements of the window's segments; null: the one segment [w0, w1) on its own
  uint64_t w0, w1;
  uint64_t n_list;            // segment starts in the list (segment j ends where j + 1 starts, the last one at w1)
  uint64_t n_seg;             // segments to take (the last of the list is left to the next window unless the range ends here)
  const uint8_t* flags;
  const uint32_t* ent;
  uint32_t P, S, K, min_cult, sense_only, fill;
  uint32_t* hist;             // K4C_GLOBAL_BLOCKS x 2 x n_entries zeroed words, or null: LDS
  uint32_t *loc, *rep, *nnz;  // the count pass's answers per segment: located, reported, entries with counts when reported
  const uint64_t *rep_pre, *dist_pre;  // fill pass: their exclusive scans
  uint64_t base_k, base_d;    // records the call wrote before this window
  k4_cult_kmer* kmers;
  uint8_t* bases;
  k4_cult_dist* dist;
};

// the P bases at a and at b are the same symbols (an offset behind the concatenation never equals a base)
K4_DEV bool k4c_same_prefix(const K4DevIndex& ix, K4Tb& ta, K4Tb& tb, uint64_t a, uint64_t b, uint32_t P) {
  if (a + P <= ix.n && b + P <= ix.n && !k4d_any_exc(ix, (int64_t)a, (int64_t)(a + P)) && !k4d_any_exc(ix, (int64_t)b, (int64_t)(b + P))) {
    for (uint32_t j = 0; j < P; j += 32) {
      const uint64_t x = k4d_ref_chunk(ix, (int64_t)(a + j)) ^ k4d_ref_chunk(ix, (int64_t)(b + j));
      if (x & k4d_range_mask(0, (int)min(32u, P - j))) return false;
    }
    return true;
  }
  for (uint32_t j = 0; j < P; j++) {
    const uint32_t x = a + j < ix.n ? ta.get((int64_t)(a + j)) : 0x10u, y = b + j < ix.n ? tb.get((int64_t)(b + j)) : 0x20u;
    if (x != y) return false;
  }
  return true;
}

// the len symbols at pos are all ACGT (:2893-2895, :3026-3028, :3119-3121)
K4_DEV bool k4c_all_acgt(const K4DevIndex& ix, K4Tb& tb, uint64_t pos, uint32_t len) {
  if (pos + len > ix.n) return false;
  if (!k4d_any_exc(ix, (int64_t)pos, (int64_t)(pos + len))) return true;
  for (uint32_t j = 0; j < len; j++)
    if (tb.get((int64_t)(pos + j)) > 3u) return false;
  return true;
}

// the block's copy of the entry table for k4d_map_entry_slow (null above K4_LDS_ENTRIES entries); a barrier follows in the caller
K4_DEV const uint64_t* k4c_entries_to_lds(const K4DevIndex& ix, uint64_t* ent_lds) {
  if (ix.n_entries > K4_LDS_ENTRIES) return nullptr;
  for (uint32_t t = threadIdx.x; t < ix.n_entries; t += blockDim.x) {
    ent_lds[t] = ix.ent_start[t];
    ent_lds[K4_LDS_ENTRIES + t] = ix.ent_end[t];
  }
  return ent_lds;
}

// F of element i and, when F, the place of its entry
template <int EL>
K4_DEV bool k4c_element(const K4DevIndex& ix, K4Tb& tb, const uint64_t* ent_lds, uint64_t i, uint32_t K, uint64_t& psn, uint32_t& en) {
  psn = k4d_sa_at<EL>(ix, i);
  en = 0xFFFFFFFFu;
  if (psn + K >= ix.n || !k4c_all_acgt(ix, tb, psn, K)) return false;
  uint64_t es, ee;
  const int e = k4d_map_entry_slow(ix, ent_lds, psn, es, ee);
  if (e < 0) return false;  // (cannot be: K bases without a separator lie inside an entry)
  en = (uint32_t)e;
  return true;
}

template <int EL>
__global__ void __launch_bounds__(256) k4k_cult_flags(K4CultFlagArgs a) {
  __shared__ uint64_t ent_mem[2 * K4_LDS_ENTRIES];
  const uint64_t* ent_lds = k4c_entries_to_lds(a.ix, ent_mem);
  __syncthreads();
  const uint64_t i = a.w0 + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= a.w1) return;
  K4Tb tb, tp;
  tb.init(a.ix);
  tp.init(a.ix);
  uint64_t psn;
  uint32_t en;
  const bool f = k4c_element<EL>(a.ix, tb, ent_lds, i, a.K, psn, en);
  bool b = i == a.forced || i == 0 || psn + a.K >= a.ix.n;
  if (!b) b = !k4c_same_prefix(a.ix, tb, tp, psn, k4d_sa_at<EL>(a.ix, i - 1), a.P);
  a.flags[i - a.w0] = (uint8_t)((b ? 1u : 0u) | (f ? 2u : 0u));
  a.ent[i - a.w0] = en;
}

template <bool LDSH>
K4_DEV uint32_t k4c_hist_get(uint32_t* p) {
  return LDSH ? *p : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDSH>
K4_DEV void k4c_hist_zero(uint32_t* p) {
  if (LDSH) *p = 0u;
  else __hip_atomic_store(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
K4_DEV uint32_t k4c_saturate(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// One wave per segment.  hist[2 e] / hist[2 e + 1] = sense / antisense counts of entry e: all zero between segments.
template <int EL, bool LDSH>
__global__ void __launch_bounds__(64) k4k_cult_segments(K4CultSegArgs a) {
  __shared__ uint64_t ent_mem[2 * K4_LDS_ENTRIES];
  __shared__ uint32_t hist_lds[LDSH ? 2 * K4C_LDS_ENTRIES : 2];
  __shared__ uint8_t pb[208];  // the head's prefix (cMaxCultivarPreSufLen = 200)
  const int lane = threadIdx.x;
  const uint32_t ne = a.ix.n_entries;
  const uint64_t* ent_lds = k4c_entries_to_lds(a.ix, ent_mem);
  uint32_t* hist = LDSH ? hist_lds : a.hist + (size_t)blockIdx.x * 2u * ne;
  if (LDSH)
    for (uint32_t t = (uint32_t)lane; t < 2u * ne; t += 64u) hist_lds[t] = 0u;
  __syncthreads();
  K4Tb tb;
  tb.init(a.ix);
  for (uint64_t seg = blockIdx.x; seg < a.n_seg; seg += gridDim.x) {
    if (a.fill && !a.rep[seg]) continue;
    const uint64_t s = a.seg_start ? a.w0 + a.seg_start[seg] : a.w0;
    const uint64_t e = a.seg_start && seg + 1 < a.n_list ? a.w0 + a.seg_start[seg + 1] : a.w1;
    // 1. the sense side: the F elements by entry, the first of them
    uint64_t n_f = 0, head = K4C_NONE;
    for (uint64_t i0 = s; i0 < e; i0 += 64) {
      const uint64_t i = i0 + (uint64_t)lane;
      if (i >= e) continue;
      bool f;
      uint32_t en;
      if (a.flags) {
        f = (a.flags[i - a.w0] & 2u) != 0;
        en = a.ent[i - a.w0];
      } else {
        uint64_t psn;
        f = k4c_element<EL>(a.ix, tb, ent_lds, i, a.K, psn, en);
      }
      if (f) {
        atomicAdd(&hist[2u * en], 1u);
        n_f++;
        if (head == K4C_NONE) head = i;
      }
    }
    n_f = k4d_wave_sum(n_f);
    head = k4d_wave_min(head);
    if (n_f == 0) continue;  // (nothing located; the count pass's answers were zeroed by the host)
    const uint64_t head_psn = k4d_sa_at<EL>(a.ix, head);
    // 2. the antisense side (AntisenseKMerCultsCnts): every occurrence of the prefix's reverse complement, kept when S ACGT bases follow
    uint64_t n_a = 0;
    if (!a.sense_only) {
      for (uint32_t j = (uint32_t)lane; j < a.P; j += 64u) pb[j] = (uint8_t)tb.get((int64_t)(head_psn + j));
      __syncthreads();
      K4QSeq qs;
      qs.q = pb; qs.len = a.P; qs.s = 1;
      uint64_t first = 0;
      uint32_t cnt = 0;
      if (lane == 0) cnt = k4q_count<EL>(a.ix, tb, qs, 0u, (int)a.P, 0xFFFFFFFFu, first);
      first = (uint64_t)__shfl((unsigned long long)first, 0, 64);
      cnt = __shfl(cnt, 0, 64);
      k4d_run_walk<EL>(a.ix, lane, first, cnt, [&](uint32_t, uint64_t pos, bool active) {
        if (!active || (a.S > 0 && !k4c_all_acgt(a.ix, tb, pos + a.P, a.S))) return false;
        uint64_t es, ee;
        const int en = k4d_map_entry_slow(a.ix, ent_lds, pos, es, ee);
        if (en < 0) return false;
        atomicAdd(&hist[2u * (uint32_t)en + 1u], 1u);
        n_a++;
        return false;
      });
      n_a = k4d_wave_sum(n_a);
    }
    __threadfence();
    __syncthreads();
    // 3. the histogram in entry order, cleared as it is read
    const bool write = a.fill != 0;
    const uint64_t k = write ? a.base_k + a.rep_pre[seg] : 0, d0 = write ? a.base_d + a.dist_pre[seg] : 0;
    uint32_t n_cult = 0;
    for (uint32_t t0 = 0; t0 < ne; t0 += 64u) {
      const uint32_t t = t0 + (uint32_t)lane;
      uint32_t sc = 0, ac = 0;
      if (t < ne) {
        sc = k4c_hist_get<LDSH>(&hist[2u * t]);
        ac = k4c_hist_get<LDSH>(&hist[2u * t + 1u]);
        if (sc) k4c_hist_zero<LDSH>(&hist[2u * t]);
        if (ac) k4c_hist_zero<LDSH>(&hist[2u * t + 1u]);
      }
      const bool nz = (sc | ac) != 0u;
      const unsigned long long m = __ballot(nz);
      if (write && nz) {
        k4_cult_dist& o = a.dist[d0 + n_cult + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))];
        o.entry_id = a.ix.ent_id[t];
        o.sense = sc;
        o.antisense = ac;
      }
      n_cult += (uint32_t)__popcll(m);
    }
    __threadfence();
    __syncthreads();
    if (!write) {
      if (lane == 0) {
        const bool reported = n_cult >= a.min_cult;
        a.loc[seg] = 1u;
        a.rep[seg] = reported ? 1u : 0u;
        a.nnz[seg] = reported ? n_cult : 0u;
      }
      continue;
    }
    if (lane == 0) {
      k4_cult_kmer& o = a.kmers[k];
      o.head_sfx_idx = head;
      o.dist_ofs = d0;
      o.sense_cnts = k4c_saturate(n_f);
      o.antisense_cnts = k4c_saturate(n_a);
      o.num_cultivars = n_cult;
      o.reserved = 0u;
    }
    for (uint32_t j = (uint32_t)lane; j < a.K; j += 64u) a.bases[k * a.K + j] = (uint8_t)tb.get((int64_t)(head_psn + j));
  }
}

// (K4S_LAUNCH_EL names a kernel by its element size alone)
template <int EL> constexpr auto k4c_segments_lds = &k4k_cult_segments<EL, true>;
template <int EL> constexpr auto k4c_segments_global = &k4k_cult_segments<EL, false>;

struct K4CultIsStart {
  const uint8_t* flags;
  __device__ bool operator()(uint32_t i) const { return (flags[i] & 1u) != 0; }
};

// ==== host side ======================================================================================================
static int check_cults_args(k4_index* ix, const k4_cults_params* p, int64_t start, int64_t end, const k4_cults_out* out, const k4_cults_caps* caps,
                            const k4_cults_totals* tot) {
  if (!ix || !p) return K4_ERR_PARAMS;
  const int64_t n = (int64_t)ix->d.n;
  const int32_t k = p->prefix_len + p->suffix_len;
  // :2846-2869
  if (p->prefix_len < 5 || p->suffix_len < 0 || p->prefix_len > 200 || p->suffix_len > 200 || p->min_cultivars < 0 || k > 300 || start < 0 ||
      end < 0 || ix->d.n_entries > K4C_MAX_CULTIVARS || (uint32_t)p->min_cultivars > ix->d.n_entries || start > n)
    return k4_fail(ix, K4_ERR_INTERNAL, "GenKMerCultsCnts: prefix %d / suffix %d / min cultivars %d / range %lld..%lld outside what %u entries and %lld elements allow",
                   p->prefix_len, p->suffix_len, p->min_cultivars, (long long)start, (long long)end, ix->d.n_entries, (long long)n);
  if (p->max_window < 0) return k4_fail(ix, K4_ERR_PARAMS, "GenKMerCultsCnts: max_window %d below 0", p->max_window);
  if (p->suffix_len > 0 && p->max_homozygotic > 0)
    return k4_fail(ix, K4_ERR_UNSUPPORTED, "GenKMerCultsCnts: the homozygotic suffix check (MaxHomozygotic %d with a suffix) is not built", p->max_homozygotic);
  if (!out || !caps || !tot || !out->kmers || !out->bases || !out->dist) return k4_fail(ix, K4_ERR_PARAMS, "GenKMerCultsCnts: null argument");
  if (caps->max_kmers < 1 || caps->max_dist < ix->d.n_entries)
    return k4_fail(ix, K4_ERR_PARAMS, "GenKMerCultsCnts: room for %llu K-mers and %llu counts, below 1 and the index's %u entries",
                   (unsigned long long)caps->max_kmers, (unsigned long long)caps->max_dist, ix->d.n_entries);
  return K4_OK;
}
// the room one call uses of the caller's caps
static k4_cults_caps cults_room(const k4_index* ix, const k4_cults_caps* caps) {
  k4_cults_caps r;
  r.max_kmers = std::min<uint64_t>(caps->max_kmers, K4C_MAX_KMERS);
  r.max_dist = std::min<uint64_t>(caps->max_dist, std::max<uint64_t>(K4C_MAX_DIST, ix->d.n_entries));
  return r;
}

namespace {
struct CultRun {
  k4_index* ix;
  K4CultState& c;
  hipStream_t st;
  uint32_t P, S, K, W;

  int begin() { return k4_check_hip(ix, c.timer.begin(st), "hipEventRecord"); }
  // the stream waited for, the section's device time added
  int lap() {
    K4_HIP(ix, c.timer.end(st));
    return k4s_call_close(ix, st, c.timer);
  }
  int reserve() {
    const size_t w = W;
    K4_HIP(ix, c.flags.reserve(w + 16));
    K4_HIP(ix, c.ent.reserve(w * 4));
    K4_HIP(ix, c.starts.reserve(w * 4 + 16));
    K4_HIP(ix, c.count.reserve(8));
    for (K4DevBuf* b : {&c.loc, &c.rep, &c.nnz}) K4_HIP(ix, b->reserve((w + 1) * 4));
    for (K4DevBuf* b : {&c.loc_pre, &c.rep_pre, &c.dist_pre}) K4_HIP(ix, b->reserve((w + 1) * 8));
    if (ix->d.n_entries > K4C_LDS_ENTRIES) {
      const size_t bytes = (size_t)K4C_GLOBAL_BLOCKS * 2 * ix->d.n_entries * 4;
      K4_HIP(ix, c.hist.reserve(bytes));
      K4_HIP(ix, hipMemsetAsync(c.hist.p, 0, bytes, st));
    }
    return K4_OK;
  }
  // b / F / entry of [w0, w1) and the window-relative segment starts; *m = how many
  int flags_and_starts(uint64_t w0, uint64_t w1, uint64_t forced, uint64_t* m) {
    K4CultFlagArgs a;
    a.ix = ix->d; a.w0 = w0; a.w1 = w1; a.forced = forced; a.P = P; a.K = K;
    a.flags = c.flags.as<uint8_t>(); a.ent = c.ent.as<uint32_t>();
    const size_t n = (size_t)(w1 - w0);
    K4_TRY(begin());
    K4S_LAUNCH_EL(ix, k4k_cult_flags, (unsigned)((n + 255) / 256), 256, st, a);
    K4_HIP(ix, hipGetLastError());
    uint32_t* out = c.starts.as<uint32_t>();
    uint64_t* d_m = c.count.as<uint64_t>();
    const K4CultIsStart pred{a.flags};
    K4_TRY(k4s_two_calls<K4DevBuf>(
        ix, "rocprim::select",
        [&](void* t, size_t& tb) { return rocprim::select(t, tb, rocprim::counting_iterator<uint32_t>(0), out, d_m, n, pred, st); }, &c.scan));
    K4_HIP(ix, hipMemcpyAsync(m, d_m, 8, hipMemcpyDeviceToHost, st));
    return lap();
  }
  void launch(const K4CultSegArgs& a) {
    const bool lds = ix->d.n_entries <= K4C_LDS_ENTRIES;
    const unsigned grid = (unsigned)std::min<uint64_t>(a.n_seg, lds ? K4C_LDS_BLOCKS : K4C_GLOBAL_BLOCKS);
    if (lds) K4S_LAUNCH_EL(ix, k4c_segments_lds, grid, 64, st, a);
    else K4S_LAUNCH_EL(ix, k4c_segments_global, grid, 64, st, a);
  }
};
}  // namespace

// The call on device outputs, its arguments checked.  Every window: flags, starts, count pass, scans, totals down, fill pass of the
// segments that fit.  A window holds no more elements than the outputs have room for K-mers and counts (a K-mer needs an element),
// so a call with small caps does a window's work in proportion to what it returns, not a full window per call; what a window
// locates beyond the room is counted again by the next call, and K4C_MIN_CAP_WINDOW bounds that.
static int cults_run(k4_index* ix, const k4_cults_params* p, int64_t start, int64_t end, const k4_cults_out* out, const k4_cults_caps* caps_in,
                     k4_cults_totals* tot, hipStream_t st) {
  K4CultState& c = ix->cul;
  const k4_cults_caps room = cults_room(ix, caps_in);
  const k4_cults_caps* caps = &room;
  K4_HIP(ix, hipSetDevice(ix->device));
  const uint64_t n = ix->d.n;
  const uint64_t last = end == 0 || (uint64_t)end >= n ? n - 1 : (uint64_t)end;  // :2871
  tot->n_located = 0; tot->n_kmers = 0; tot->n_dist = 0; tot->next_sfx_idx = (uint64_t)start; tot->done = 1;
  if ((uint64_t)start > last) return K4_OK;
  CultRun r{ix, c, st, (uint32_t)p->prefix_len, (uint32_t)p->suffix_len, (uint32_t)(p->prefix_len + p->suffix_len),
            p->max_window == 0 ? K4C_DEFAULT_WINDOW : (uint32_t)std::min<int64_t>(p->max_window, K4C_MAX_WINDOW)};
  r.W = (uint32_t)std::min<uint64_t>(r.W, last + 1 - (uint64_t)start);
  const uint32_t full_window = r.W;
  K4_TRY(r.reserve());
  const uint32_t min_cult = p->min_cultivars == 0 ? ix->d.n_entries : (uint32_t)p->min_cultivars;  // :2865
  uint64_t cur = (uint64_t)start;
  std::vector<uint64_t> h_rep, h_dist, h_loc;
  bool full = false;
  while (cur <= last && !full) {
    const uint64_t left = std::min<uint64_t>(caps->max_kmers - tot->n_kmers, caps->max_dist - tot->n_dist);
    r.W = (uint32_t)std::min<uint64_t>(full_window, std::max<uint64_t>(left, K4C_MIN_CAP_WINDOW));
    uint64_t w1 = std::min<uint64_t>(cur + r.W, last + 1), m = 0;
    K4_TRY(r.flags_and_starts(cur, w1, cur, &m));
    const bool final_window = w1 == last + 1;
    K4CultSegArgs a;
    a.ix = ix->d; a.w0 = cur; a.P = r.P; a.S = r.S; a.K = r.K; a.min_cult = min_cult; a.sense_only = p->sense_only ? 1u : 0u;
    a.hist = ix->d.n_entries > K4C_LDS_ENTRIES ? c.hist.as<uint32_t>() : nullptr;
    a.loc = c.loc.as<uint32_t>(); a.rep = c.rep.as<uint32_t>(); a.nnz = c.nnz.as<uint32_t>();
    a.rep_pre = c.rep_pre.as<uint64_t>(); a.dist_pre = c.dist_pre.as<uint64_t>();
    a.kmers = out->kmers; a.bases = out->bases; a.dist = out->dist;
    uint64_t next;
    if (m >= 2 || final_window) {  // (the window's first element is a start: m >= 1)
      a.seg_start = c.starts.as<uint32_t>(); a.flags = c.flags.as<uint8_t>(); a.ent = c.ent.as<uint32_t>();
      a.w1 = w1; a.n_list = m; a.n_seg = final_window ? m : m - 1;
      next = w1;  // (unless the last segment is left over: its start comes down with the totals)
    } else {  // one segment fills the window and goes on: its end is the next start, looked for window by window
      uint64_t e = last + 1;
      for (uint64_t w = w1; w <= last; w += r.W) {
        uint64_t m2 = 0;
        K4_TRY(r.flags_and_starts(w, std::min<uint64_t>(w + r.W, last + 1), K4C_NONE, &m2));
        if (m2 > 0) {
          uint32_t first = 0;
          K4_TRY(k4s_read_back(ix, &first, c.starts.p, st));
          e = w + first;
          break;
        }
      }
      a.seg_start = nullptr; a.flags = nullptr; a.ent = nullptr;
      a.w1 = e; a.n_list = 1; a.n_seg = 1;
      next = e;
    }
    uint32_t left_over = 0;
    if (a.seg_start && a.n_seg < m) K4_HIP(ix, hipMemcpyAsync(&left_over, c.starts.as<uint32_t>() + (m - 1), 4, hipMemcpyDeviceToHost, st));
    const size_t ns = (size_t)a.n_seg;
    for (K4DevBuf* b : {&c.loc, &c.rep, &c.nnz}) K4_HIP(ix, hipMemsetAsync(b->p, 0, (ns + 1) * 4, st));
    K4_TRY(r.begin());
    a.fill = 0; a.base_k = 0; a.base_d = 0;
    r.launch(a);
    K4_HIP(ix, hipGetLastError());
    K4_TRY(k4s_exclusive_scan(ix, c.loc.as<uint32_t>(), c.loc_pre.as<uint64_t>(), (uint64_t)0, ns + 1, rocprim::plus<uint64_t>(), st, &c.scan));
    K4_TRY(k4s_exclusive_scan(ix, c.rep.as<uint32_t>(), c.rep_pre.as<uint64_t>(), (uint64_t)0, ns + 1, rocprim::plus<uint64_t>(), st, &c.scan));
    K4_TRY(k4s_exclusive_scan(ix, c.nnz.as<uint32_t>(), c.dist_pre.as<uint64_t>(), (uint64_t)0, ns + 1, rocprim::plus<uint64_t>(), st, &c.scan));
    uint64_t t3[3] = {0, 0, 0};
    K4_HIP(ix, hipMemcpyAsync(&t3[0], c.loc_pre.as<uint64_t>() + ns, 8, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipMemcpyAsync(&t3[1], c.rep_pre.as<uint64_t>() + ns, 8, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipMemcpyAsync(&t3[2], c.dist_pre.as<uint64_t>() + ns, 8, hipMemcpyDeviceToHost, st));
    K4_TRY(r.lap());
    if (a.seg_start && a.n_seg < m) next = cur + left_over;
    uint64_t take = ns;
    if (tot->n_kmers + t3[1] > caps->max_kmers || tot->n_dist + t3[2] > caps->max_dist) {
      // the outputs cannot hold the window: the longest run of whole segments that fits; the call ends in front of the next one
      full = true;
      h_loc.resize(ns + 1); h_rep.resize(ns + 1); h_dist.resize(ns + 1);
      K4_HIP(ix, hipMemcpyAsync(h_loc.data(), c.loc_pre.p, (ns + 1) * 8, hipMemcpyDeviceToHost, st));
      K4_HIP(ix, hipMemcpyAsync(h_rep.data(), c.rep_pre.p, (ns + 1) * 8, hipMemcpyDeviceToHost, st));
      K4_HIP(ix, hipMemcpyAsync(h_dist.data(), c.dist_pre.p, (ns + 1) * 8, hipMemcpyDeviceToHost, st));
      K4_HIP(ix, hipStreamSynchronize(st));
      take = 0;
      while (take < ns && tot->n_kmers + h_rep[take + 1] <= caps->max_kmers && tot->n_dist + h_dist[take + 1] <= caps->max_dist) take++;
      t3[0] = h_loc[take]; t3[1] = h_rep[take]; t3[2] = h_dist[take];
      if (a.seg_start) {
        uint32_t s_take = 0;
        K4_TRY(k4s_read_back(ix, &s_take, c.starts.as<uint32_t>() + take, st));
        next = cur + s_take;
      } else
        next = cur;
    }
    if (t3[1] > 0) {
      K4_TRY(r.begin());
      a.fill = 1; a.n_seg = take; a.base_k = tot->n_kmers; a.base_d = tot->n_dist;
      r.launch(a);
      K4_HIP(ix, hipGetLastError());
      K4_TRY(r.lap());
    }
    tot->n_located += (int64_t)t3[0]; tot->n_kmers += t3[1]; tot->n_dist += t3[2];
    cur = next;
  }
  tot->next_sfx_idx = cur;
  tot->done = cur > last ? 1 : 0;
  return K4_OK;
}

extern "C" int k4_kmer_cults_batch_dev(k4_index* ix, const k4_cults_params* p, int64_t start_sfx_idx, int64_t end_sfx_idx, const k4_cults_out* d_out,
                                       const k4_cults_caps* caps, k4_cults_totals* totals, void* stream) {
  if (ix) ix->cul.timer.reset();
  const int rc = check_cults_args(ix, p, start_sfx_idx, end_sfx_idx, d_out, caps, totals);
  return rc != K4_OK ? rc : cults_run(ix, p, start_sfx_idx, end_sfx_idx, d_out, caps, totals, (hipStream_t)stream);
}

// host outputs: the records are staged on the device in room for the caps, and what was written comes back; nothing else is touched
extern "C" int k4_kmer_cults_batch(k4_index* ix, const k4_cults_params* p, int64_t start_sfx_idx, int64_t end_sfx_idx, const k4_cults_out* out,
                                   const k4_cults_caps* caps, k4_cults_totals* totals) {
  if (ix) ix->cul.timer.reset();
  int rc = check_cults_args(ix, p, start_sfx_idx, end_sfx_idx, out, caps, totals);
  if (rc != K4_OK) return rc;
  K4CultState& c = ix->cul;
  const k4_cults_caps room = cults_room(ix, caps);
  const size_t klen = (size_t)(p->prefix_len + p->suffix_len);
  hipStream_t st;
  K4_TRY(k4s_call_open(ix, &st));
  K4_HIP(ix, c.out_kmers.reserve((size_t)room.max_kmers * sizeof(k4_cult_kmer) + 16));
  K4_HIP(ix, c.out_bases.reserve((size_t)room.max_kmers * klen + 16));
  K4_HIP(ix, c.out_dist.reserve((size_t)room.max_dist * sizeof(k4_cult_dist) + 16));
  k4_cults_out d;
  d.kmers = c.out_kmers.as<k4_cult_kmer>(); d.bases = c.out_bases.as<uint8_t>(); d.dist = c.out_dist.as<k4_cult_dist>();
  if ((rc = cults_run(ix, p, start_sfx_idx, end_sfx_idx, &d, caps, totals, st)) != K4_OK) return rc;
  if (totals->n_kmers) {
    K4_HIP(ix, hipMemcpyAsync(out->kmers, d.kmers, (size_t)totals->n_kmers * sizeof(k4_cult_kmer), hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipMemcpyAsync(out->bases, d.bases, (size_t)totals->n_kmers * klen, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipMemcpyAsync(out->dist, d.dist, (size_t)totals->n_dist * sizeof(k4_cult_dist), hipMemcpyDeviceToHost, st));
  }
  return k4s_call_close(ix, st, c.timer);
}

extern "C" double k4_cults_last_kernel_ms(const k4_index* ix) { return ix ? ix->cul.timer.ms : 0.0; }

// SfxOfsToLoci (SfxArray.cpp:49-60) for n elements from `first`
extern "C" int k4_get_sfx_els(k4_index* ix, uint64_t first, uint64_t n, uint64_t* els) {
  if (!ix || (n > 0 && !els)) return K4_ERR_PARAMS;
  if (first > ix->d.n || n > ix->d.n - first) return k4_fail(ix, K4_ERR_PARAMS, "k4_get_sfx_els: %llu elements from %llu leave the array", (unsigned long long)n, (unsigned long long)first);
  if (n == 0) return K4_OK;
  K4_HIP(ix, hipSetDevice(ix->device));
  const uint32_t el = ix->d.el;
  std::vector<uint8_t> raw((size_t)n * el);
  K4_HIP(ix, hipMemcpy(raw.data(), ix->d.sa + first * el, raw.size(), hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < n; i++) {
    uint64_t v = 0;
    for (uint32_t b = 0; b < el; b++) v |= (uint64_t)raw[(size_t)i * el + b] << (8 * b);
    els[i] = v;
  }
  return K4_OK;
}
