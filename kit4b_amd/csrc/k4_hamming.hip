// kit4b_amd/csrc/k4_hamming.hip -- CSfxArray::LocateSfxHammings / LocateHammings over LocateHamming (libkit4b/SfxArray.cpp:4107-4627,
// `ngskit4b hammings -m0`) on gfx950: one WAVE per sampled K-mer.  The K-mer sits in LDS with its N substituted; a stage of the
// escalation is LocateHamming itself: the exact pass over the run of the whole K-mer, then per strand the segments' runs resolved one
// per lane (k-mer table bucket, bounds no further than the depth that can be explored), the (segment, occurrence) candidates laid
// out in the reference's order by a prefix sum and taken 64 at a time.  A lane counts its candidate's mismatches against the
// CurHamming of the chunk's start; the first lane in order that brings it to RHammMin or below ends the stage, otherwise the
// wave's minimum is the new CurHamming.  DESIGN.md "Restricted Hammings" has the rest.
#include <algorithm>
#include "k4_stage.h"

#define K4H_MAX_KMER 500
#define K4H_LAUNCH_KMERS 32768  // K-mers (waves) per launch: at the `ultra` preset one core may walk 500 000 suffixes
#define K4H_SKIP 0xFFFFu        // a candidate the reference passes over

struct K4HSpan {
  uint64_t src;    // sfx form: concatenation offset of the span's first base; seq form: offset into seqs
  uint64_t out;    // the span's first byte in hammings
  uint64_t kbase;  // sampled K-mers of the spans in front (the table ends with a sentinel that holds the total)
  uint32_t entry_id, loci;
};

struct K4HammArgs {
  K4DevIndex ix;
  const K4HSpan* spans;
  int64_t n_spans;
  const uint8_t* seqs;  // null: the sfx form
  uint8_t* out;
  uint64_t k0, k1;  // this launch's K-mers
  k4_hamming_params p;
};

// is an exact match at locus loci of target tid one the reference passes over (:4411-4452, :4585-4601): the probe itself, which
// only a sense pass knows, or a target the intra / inter filter leaves out
K4_DEV bool k4h_filtered(uint32_t tid, uint32_t loci, uint32_t probe_entry, uint32_t probe_loci, int iib, bool sense) {
  if (sense && tid == probe_entry && loci == probe_loci) return true;
  return (iib == 1 && tid != probe_entry) || (iib == 2 && tid == probe_entry);
}

// one candidate of segment seg (LocateHamming :4533-4601): the suffix at pos holds the segment's core.  The mismatches of the
// K-mer window around it, or K4H_SKIP.  The duplicate-segment test (:4546-4561) rides on the count: an earlier segment without a
// mismatch is an earlier segment that matches exactly, and a window the count gives up on is passed over either way.
K4_DEV uint32_t k4h_candidate(const K4DevIndex& ix, K4Tb& tb, const K4QSeq& qs, uint32_t core_len, uint32_t seg, uint64_t pos, uint32_t thr,
                              bool sense, uint32_t probe_entry, uint32_t probe_loci, int iib) {
  const uint32_t seg_ofs = seg * core_len;
  if (pos < seg_ofs) return K4H_SKIP;
  const uint64_t left = pos - seg_ofs;
  if (left + qs.len > ix.n) return K4H_SKIP;
  uint32_t mm = 0, seg_mm = 0, d = 0, in_seg = 0;
  for (uint32_t j = 0; j < qs.len; j++) {
    const uint32_t t = tb.get((int64_t)(left + j));
    if (t == 7u) return K4H_SKIP;  // (an EOS inside an earlier segment ends CmpProbeTarg below zero: no duplicate, and the count ends here)
    if (qs.at(j) != t) {
      if (++mm > thr) return K4H_SKIP;
      seg_mm++;
    }
    if (++in_seg == core_len) {
      if (d < seg && seg_mm == 0) return K4H_SKIP;
      d++; in_seg = 0; seg_mm = 0;
    }
  }
  if (mm == 0 && sense && probe_entry > 0) {  // :4585-4601
    const int e = k4d_map_entry(ix, left);
    if (e >= 0 && k4h_filtered(ix.ent_id[e], (uint32_t)(left - ix.ent_start[e]), probe_entry, probe_loci, iib, sense)) return K4H_SKIP;
  }
  return mm;
}

// LocateHamming (:4339-4627) by one wave; pb = the K-mer (no N left in it).  Every lane returns the same value.
template <int EL>
K4_DEV uint32_t k4h_locate(const K4DevIndex& ix, K4Tb& tb, const uint8_t* pb, uint32_t len, uint32_t hmin, uint32_t hmax, uint32_t min_cd,
                           uint32_t max_cd, bool both, uint32_t probe_entry, uint32_t probe_loci, int iib, uint64_t* g_first, uint32_t* g_pre) {
  const int lane = threadIdx.x;
  K4QSeq qs;
  qs.q = pb; qs.len = len;
  if (hmin == 0) {  // :4411-4452: IterateExacts on the whole K-mer, sense then antisense
    const int ns = both ? 2 : 1;
    uint64_t first;
    const uint32_t cnt = k4d_cores_to_lanes<EL>(
        ix, tb, lane, (uint32_t)ns, 1u, len, 0xFFFFFFFFu, [&](uint32_t s) { return K4QSeq{pb, len, (int)s}; }, [](uint32_t) { return 0u; }, first);
    for (int s = 0; s < ns; s++) {
      const uint32_t c = __shfl(cnt, s, 64);
      const bool filtered = s == 0 ? probe_entry != 0 : (probe_entry != 0 && iib != 0);
      if (c && !filtered) return 0u;
      const bool kept = k4d_run_walk<EL>(ix, lane, __shfl(first, s, 64), c, [&](uint32_t, uint64_t pos, bool active) {
        const int e = active ? k4d_map_entry(ix, pos) : -1;
        // (the antisense run holds no self hit)
        return e >= 0 && !k4h_filtered(ix.ent_id[e], (uint32_t)(pos - ix.ent_start[e]), probe_entry, probe_loci, iib, s == 0);
      });
      if (kept) return 0u;
    }
  }
  if (hmax == 0) return 1u;
  const uint32_t core_len = len / (hmax + 1), n_seg = len / core_len;
  uint32_t cur = n_seg;
  const uint32_t cap = (uint32_t)min((uint64_t)max_cd + (uint64_t)min_cd, (uint64_t)0xFFFFFFFFull);
  for (int s = 0; s < (both ? 2 : 1) && cur > hmin; s++) {
    qs.s = s;
    // 1. one segment per lane: first index of its run and the occurrences the reference's walk reaches.  The walk takes at most
    // max_cd of them; on its min_cd-th turn it counts the run once and gives the segment up when what is left, as it counts it
    // (run + 3 - min_cd), exceeds max_cd (:4487-4494)
    uint64_t first;
    const uint32_t run = k4d_cores_to_lanes<EL>(
        ix, tb, lane, max_cd > 0 ? n_seg : 0u, n_seg, core_len, cap, [&](uint32_t) { return qs; }, [&](uint32_t seg) { return seg * core_len; }, first);
    uint32_t take = min(run, max_cd);
    if (min_cd >= 2 && min_cd <= max_cd && (uint64_t)run + 1 >= min_cd && (uint64_t)run + 3 > (uint64_t)max_cd + min_cd) take = min_cd - 1;
    __syncthreads();  // (the previous pass has done with g_first / g_pre)
    k4d_runs_layout(lane, first, take, g_first, g_pre);
    __syncthreads();
    const uint32_t total = g_pre[64];
    // 2. the candidates in the reference's order, 64 at a time
    for (uint32_t c0 = 0; c0 < total && cur > hmin; c0 += 64) {
      const uint32_t g = c0 + (uint32_t)lane;
      uint32_t mm = K4H_SKIP;
      if (g < total) {
        uint32_t seg, occ;
        k4d_runs_locate(g, n_seg - 1, g_pre, seg, occ);
        const uint64_t pos = k4d_sa_at<EL>(ix, g_first[seg] + occ);
        mm = k4h_candidate(ix, tb, qs, core_len, seg, pos, cur, s == 0, probe_entry, probe_loci, iib);
      }
      // 3. in order: the first candidate at or under hmin ends the stage (nothing in front of it was), else the minimum stands
      const unsigned long long stop = __ballot(mm != K4H_SKIP && mm <= hmin);
      if (stop) return __shfl(mm, __ffsll((long long)stop) - 1, 64);
      cur = min(cur, k4d_wave_min(mm));
    }
    probe_entry = 0;  // :4617: the antisense pass knows no self hit
  }
  return cur;
}

template <int EL>
__global__ void __launch_bounds__(64) k4k_hammings(K4HammArgs a) {
  __shared__ uint8_t pb[512];
  __shared__ uint32_t n_idx[8];
  __shared__ uint64_t g_first[64];
  __shared__ uint32_t g_pre[65];
  const int lane = threadIdx.x;
  const uint64_t kid = a.k0 + blockIdx.x;
  if (kid >= a.k1) return;
  const K4HSpan sp = a.spans[k4d_last_le(a.n_spans, kid, [&](int64_t i) { return a.spans[i].kbase; })];  // the span that holds K-mer kid
  const k4_hamming_params p = a.p;
  const uint32_t len = (uint32_t)p.kmer_len, nth = (uint32_t)p.sample_nth;
  const uint32_t ofs = (uint32_t)(kid - sp.kbase) * nth;
  K4Tb tb;
  tb.init(a.ix);
  uint32_t n_ns = 0;  // (an EOS counts with the N, :4157)
  for (uint32_t j0 = 0; j0 < len; j0 += 64) {
    const uint32_t j = j0 + (uint32_t)lane;
    uint32_t b = 0;
    if (j < len) {
      b = a.seqs ? (a.seqs[sp.src + ofs + j] & 0x0fu) : tb.get((int64_t)(sp.src + ofs + j));
      pb[j] = (uint8_t)b;
    }
    const bool is_n = j < len && b >= 4u;
    const unsigned long long m = __ballot(is_n);
    if (is_n) {
      const uint32_t r = n_ns + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (r < 8) n_idx[r] = j;
    }
    n_ns += (uint32_t)__popcll(m);
  }
  __syncthreads();
  uint32_t lowest = 0;
  if (n_ns <= 4) {
    const uint32_t probe_entry = a.seqs ? 0u : sp.entry_id, probe_loci = a.seqs ? ofs : sp.loci + ofs;
    const uint32_t rh = (uint32_t)p.rhamm, mn = p.min_core_depth, mx = p.max_core_depth;
    const bool both = p.both_strands != 0;
    const uint32_t n_iters = 1u << (2 * n_ns);
    lowest = 0x7f;
    for (uint32_t it = 0; it < n_iters && lowest != 0; it++) {
      if ((uint32_t)lane < n_ns) pb[n_idx[lane]] = (uint8_t)((it >> (2 * lane)) & 3u);
      __syncthreads();
      // :4185-4199: the depths are products of 32-bit unsigned values in the reference as well
      uint32_t r = k4h_locate<EL>(a.ix, tb, pb, len, 0, 1, 2 * mn, 10 * mx, both, probe_entry, probe_loci, p.intra_inter_both, g_first, g_pre);
      if (r > 1 && rh > 1) {
        r = k4h_locate<EL>(a.ix, tb, pb, len, 2, 2, 2 * mn, 8 * mx, both, probe_entry, probe_loci, p.intra_inter_both, g_first, g_pre);
        if (r > 2 && rh > 2) {
          r = k4h_locate<EL>(a.ix, tb, pb, len, 3, 3, 2 * mn, 4 * mx, both, probe_entry, probe_loci, p.intra_inter_both, g_first, g_pre);
          if (r > 3 && rh > 3) {
            r = k4h_locate<EL>(a.ix, tb, pb, len, 4, 4, mn, 2 * mx, both, probe_entry, probe_loci, p.intra_inter_both, g_first, g_pre);
            if (r > 4 && rh > 4)
              r = k4h_locate<EL>(a.ix, tb, pb, len, 5, rh, mn, mx, both, probe_entry, probe_loci, p.intra_inter_both, g_first, g_pre);
          }
        }
      }
      if ((r & 0x7fu) < lowest) lowest = r & 0x7fu;
      __syncthreads();  // (pb is rewritten by the next substitution)
    }
    if (!a.seqs && lowest > 20) lowest = 20;  // :4208; LocateHammings has no clamp
  }
  if (lane == 0) a.out[sp.out + ofs] = (uint8_t)lowest;
}

// ==== host side ======================================================================================================
static int check_hamming_params(k4_index* ix, const k4_hamming_params* p) {
  if (!ix || !p) return K4_ERR_PARAMS;
  if (p->rhamm < 1 || p->kmer_len < 10 || p->kmer_len > K4H_MAX_KMER)
    return k4_fail(ix, K4_ERR_INTERNAL, "Hammings: rhamm %d below 1 or kmer_len %d outside 10..500", p->rhamm, p->kmer_len);
  if (p->rhamm > 10) return k4_fail(ix, K4_ERR_PARAMS, "Hammings: rhamm %d above 10", p->rhamm);
  if (p->kmer_len / (p->rhamm + 1) < 8)
    return k4_fail(ix, K4_ERR_PARAMS, "Hammings: kmer_len %d / (rhamm %d + 1) is a core under 8 bases", p->kmer_len, p->rhamm);
  if (p->intra_inter_both < 0 || p->intra_inter_both > 2)
    return k4_fail(ix, K4_ERR_PARAMS, "Hammings: intra_inter_both %d outside 0..2", p->intra_inter_both);
  return K4_OK;
}

// the span table of a batch; sfx form when entry_ids is given, else the seq form over offs / lens
static int hamming_spans(k4_index* ix, const k4_hamming_params* p, int64_t n, const uint32_t* entry_ids, const uint32_t* entry_locis,
                         const uint32_t* span_lens, const uint64_t* offs, const uint64_t* out_offs, uint64_t out_len, std::vector<K4HSpan>& t) {
  const uint32_t klen = (uint32_t)p->kmer_len, nth = p->sample_nth > 0 ? (uint32_t)p->sample_nth : 1u;
  uint64_t kbase = 0;
  t.resize((size_t)n + 1);
  for (int64_t i = 0; i < n; i++) {
    const uint32_t sl = span_lens[i];
    if (sl < klen) return k4_fail(ix, K4_ERR_INTERNAL, "Hammings: span %lld of %u bases is shorter than kmer_len %u", (long long)i, sl, klen);
    K4HSpan& s = t[(size_t)i];
    if (entry_ids) {
      const k4_entry* e = k4i_entry_by_id(ix, entry_ids[i]);
      if (!e || e->seq_len == 0 || entry_locis[i] > e->seq_len || e->seq_len - entry_locis[i] < sl)
        return k4_fail(ix, K4_ERR_INTERNAL, "Hammings: span %lld (entry %u, locus %u, %u bases) is not inside an entry", (long long)i,
                       entry_ids[i], entry_locis[i], sl);
      s.src = e->start_ofs + entry_locis[i];
      s.entry_id = entry_ids[i]; s.loci = entry_locis[i];
    } else {
      s.src = offs[i];
      s.entry_id = 0; s.loci = 0;
    }
    const uint64_t last = (uint64_t)((sl - klen) / nth) * nth;
    if (out_offs[i] > out_len || last >= out_len - out_offs[i])
      return k4_fail(ix, K4_ERR_PARAMS, "Hammings: span %lld writes past hammings_len %llu", (long long)i, (unsigned long long)out_len);
    s.out = out_offs[i];
    s.kbase = kbase;
    kbase += (uint64_t)(sl - klen) / nth + 1;
  }
  K4HSpan& z = t[(size_t)n];
  z.src = z.out = 0; z.kbase = kbase; z.entry_id = z.loci = 0;
  return K4_OK;
}

// One batch, for the four entry points.  sfx: the spans are (entry_ids, entry_locis, lens) of the index itself and seqs / offs stay
// null; otherwise they are the lens[i] bases at seqs + offs[i].  on_host: seqs and hammings are the caller's own arrays and the
// index's stream is used; hammings then goes up whole and comes back whole, so the bytes no K-mer owns return as they came.
static int hamming_batch(k4_index* ix, const k4_hamming_params* p, bool sfx, bool on_host, int64_t n, const uint32_t* entry_ids,
                         const uint32_t* entry_locis, const void* seqs, const uint64_t* offs, const uint32_t* lens, const uint64_t* out_offs,
                         void* hammings, uint64_t hammings_len, hipStream_t st) {
  int rc = check_hamming_params(ix, p);
  if (rc != K4_OK) return rc;
  K4HammState& h = ix->hmm;
  h.timer.reset();
  const bool src = sfx ? n == 0 || (entry_ids && entry_locis) : seqs && (n == 0 || offs);
  if (n < 0 || !hammings || !src || (n > 0 && (!lens || !out_offs))) return k4_fail(ix, K4_ERR_INTERNAL, "Hammings: null argument");
  std::vector<K4HSpan> t;
  if ((rc = hamming_spans(ix, p, n, entry_ids, entry_locis, lens, offs, out_offs, hammings_len, t)) != K4_OK) return rc;
  const uint64_t total = t[(size_t)n].kbase;
  if (total == 0) return K4_OK;
  K4HammArgs a;
  a.seqs = (const uint8_t*)seqs;  // (null: the sfx form)
  a.out = (uint8_t*)hammings;
  if (!on_host) {
    K4_HIP(ix, hipSetDevice(ix->device));
    K4_HIP(ix, hipStreamSynchronize(st));  // (the span table about to be replaced may still be read by the batch before)
  } else {
    K4_TRY(k4s_call_open(ix, &st));
    K4_HIP(ix, h.out.reserve((size_t)hammings_len + 16));
    K4_HIP(ix, hipMemcpyAsync(h.out.p, hammings, (size_t)hammings_len, hipMemcpyHostToDevice, st));
    if (!sfx) K4_TRY(k4s_stage_seqs(ix, n, (const uint8_t*)seqs, offs, lens, nullptr));
    a.seqs = sfx ? nullptr : ix->seq_stage.seqs.as<uint8_t>();
    a.out = h.out.as<uint8_t>();
  }
  K4_HIP(ix, h.spans.reserve(t.size() * sizeof(K4HSpan)));
  K4_HIP(ix, hipMemcpyAsync(h.spans.p, t.data(), t.size() * sizeof(K4HSpan), hipMemcpyHostToDevice, st));
  a.ix = ix->d;
  a.spans = h.spans.as<K4HSpan>();
  a.n_spans = n;
  a.p = *p;
  if (a.p.sample_nth <= 0) a.p.sample_nth = 1;
  K4_HIP(ix, h.timer.begin(st));
  k4s_launch_windows(total, K4H_LAUNCH_KMERS, [&](uint64_t k0, uint64_t k1) {
    a.k0 = k0;
    a.k1 = k1;
    K4S_LAUNCH_EL(ix, k4k_hammings, (unsigned)(k1 - k0), 64, st, a);
  });
  K4_HIP(ix, hipGetLastError());
  K4_HIP(ix, h.timer.end(st));
  if (on_host) K4_HIP(ix, hipMemcpyAsync(hammings, h.out.p, (size_t)hammings_len, hipMemcpyDeviceToHost, st));
  return k4s_call_close(ix, st, h.timer);
}

extern "C" int k4_locate_sfx_hammings_batch_dev(k4_index* ix, const k4_hamming_params* p, int64_t n, const uint32_t* entry_ids,
                                                const uint32_t* entry_locis, const uint32_t* span_lens, const uint64_t* out_offs,
                                                void* d_hammings, uint64_t hammings_len, void* stream) {
  return hamming_batch(ix, p, true, false, n, entry_ids, entry_locis, nullptr, nullptr, span_lens, out_offs, d_hammings, hammings_len,
                       (hipStream_t)stream);
}

extern "C" int k4_locate_hammings_batch_dev(k4_index* ix, const k4_hamming_params* p, int64_t n, const void* d_seqs, const uint64_t* offs,
                                            const uint32_t* lens, const uint64_t* out_offs, void* d_hammings, uint64_t hammings_len,
                                            void* stream) {
  return hamming_batch(ix, p, false, false, n, nullptr, nullptr, d_seqs, offs, lens, out_offs, d_hammings, hammings_len, (hipStream_t)stream);
}

extern "C" int k4_locate_sfx_hammings_batch(k4_index* ix, const k4_hamming_params* p, int64_t n, const uint32_t* entry_ids,
                                            const uint32_t* entry_locis, const uint32_t* span_lens, const uint64_t* out_offs, uint8_t* hammings,
                                            uint64_t hammings_len) {
  return hamming_batch(ix, p, true, true, n, entry_ids, entry_locis, nullptr, nullptr, span_lens, out_offs, hammings, hammings_len, nullptr);
}

extern "C" int k4_locate_hammings_batch(k4_index* ix, const k4_hamming_params* p, int64_t n, const uint8_t* seqs, const uint64_t* offs,
                                        const uint32_t* lens, const uint64_t* out_offs, uint8_t* hammings, uint64_t hammings_len) {
  return hamming_batch(ix, p, false, true, n, nullptr, nullptr, seqs, offs, lens, out_offs, hammings, hammings_len, nullptr);
}

extern "C" double k4_hamming_last_kernel_ms(const k4_index* ix) { return ix ? ix->hmm.timer.ms : 0.0; }

