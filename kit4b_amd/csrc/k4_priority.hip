// kit4b_amd/csrc/k4_priority.hip -- `kalign -B <bed>` / `-V`: priority regions.
//   k4_set_priority_regions          <- what CKAligner::Align keeps of its CBEDfile (ngskit4b/KAligner.cpp:311-330): per sequence of the
//                                       index the loci some feature covers (CBEDfile::InAnyFeature, libkit4b/BEDfile.cpp:3991,3247-3306)
//   k4i_priority_kalign              <- the priority pass of CKAligner::ProcCoredApprox (:9682-9770) in front of the normal call (:9774-9817)
//   k4_filter_priority_regions_dev   <- CKAligner::FiltByPriorityRegions (:4093-4155)
//
// The reference gives every read an AlignReads call with MaxML + cPriorityExacts (10) hits, no microInDel and no splice phase, walks
// the hits it reported, keeps those that lie in a feature (in order) and, when there are between 1 and MaxML of them, goes on with
// them and with the LowMMCnt / NxtLowMMCnt of that call; every other read gets the normal call.  Here, per batch:
//   (a) the alignment kernels with max_ml + 10 into a scratch result / hit set            (k4i_kalign_core, all reads)
//   (b) k4k_priority_select, a lane per read: span test per hit, compaction into the caller's hit slots, the acceptance rule with
//       AlignRead's classification of an eHRhits result, and a mark for the reads that need the normal call
//   (c) the marked reads listed (k4s_select_indices), their offsets / lengths gathered, the alignment kernels over them alone
//   (d) k4k_priority_scatter: the normal call's records into the caller's arrays at the reads' places
// A span test is one binary search: the intervals of a sequence are sorted, disjoint and inclusive, so [s, e] meets a feature iff the
// first interval that ends at or behind s starts at or before e.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <utility>
#include <vector>
#include "k4_device.h"
#include "k4_stage.h"

#define K4_PRIORITY_EXACTS 10  /* cPriorityExacts, KAligner.h:58 */

namespace {

struct K4PriTab {
  const uint32_t* off;    // n_entries + 2 words: the intervals of entry id c are [off[c], off[c + 1])
  const uint32_t* start;
  const uint32_t* end;
  const uint32_t* pt_off;  // n_entries + 2 words: the features of no bases of entry id c are pt[pt_off[c] .. pt_off[c + 1]), ascending
  const uint32_t* pt;      // Start of such a feature (its End is Start - 1): met by a span that covers Start - 1 and Start
  uint32_t n_entries;
};

// InAnyFeature(sequence c, s, e): 0-based inclusive loci, any strand
K4_DEV bool k4d_in_feature(const K4PriTab& t, uint32_t c, uint32_t s, uint32_t e) {
  if (c < 1 || c > t.n_entries) return false;  // (GetIdentName fails: not a priority hit)
  uint32_t lo = t.off[c];
  const uint32_t top = t.off[c + 1];
  uint32_t hi = top;
  while (lo < hi) {  // the first interval with end >= s
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (t.end[mid] < s) lo = mid + 1; else hi = mid;
  }
  if (lo < top && t.start[lo] <= e) return true;
  lo = t.pt_off[c];
  const uint32_t ptop = t.pt_off[c + 1];
  hi = ptop;
  while (lo < hi) {  // the first point behind s: Start <= e && Start - 1 >= s
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (t.pt[mid] <= s) lo = mid + 1; else hi = mid;
  }
  return lo < ptop && t.pt[lo] <= e;
}

K4_DEV bool k4d_hit_in_feature(const K4PriTab& t, const k4_hit& h) {
  return k4d_in_feature(t, h.chrom_id, h.match_loci, h.match_loci + (uint32_t)h.match_len - 1u);  // the raw MatchLoci / MatchLen
}

// (b): wide = the records of the call with max_ml + 10 hit slots.  need[i] = 1: the read gets the normal call.
__global__ void __launch_bounds__(256) k4k_priority_select(K4PriTab t, int64_t n, int max_ml, int pe_mode, int sparse_hits,
                                                           const k4_read_result* __restrict__ wide_rr, const k4_hit* __restrict__ wide_hits,
                                                           k4_read_result* __restrict__ out_rr, k4_hit* __restrict__ out_hits,
                                                           uint8_t* __restrict__ need) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int wide_ml = max_ml + K4_PRIORITY_EXACTS;
  const k4_read_result w = wide_rr[i];
  int n_pri = 0;
  if (w.hit_rslt == K4_HR_HITS) {
    const k4_hit* src = wide_hits + i * wide_ml;
    k4_hit* dst = out_hits + i * max_ml;
    const int walk = min(w.inst, wide_ml);
    // The compaction of :9732-9755 as it is written: the hits stay where AlignReads put them, and a priority hit is copied to
    // the front -- to a slot counter that starts at 0 and moves with the COPIES only -- once a hit outside the regions has been
    // passed.  So the priority hits in front of the first outsider are not counted into that slot: [P1, N, P2] ends as
    // [P2, N, ...] with two instances, and the outsider N is reported as the second.  (A copy goes to a slot in front of the
    // hit it reads, so reading from the untouched wide set gives what the reference's in-place walk gives.)
    int n_out = 0, n_copied = 0;
    for (int q = 0; q < walk; q++) {
      const uint4 v = *reinterpret_cast<const uint4*>(&src[q]);
      k4_hit h;
      *reinterpret_cast<uint4*>(&h) = v;
      if (q < max_ml) *reinterpret_cast<uint4*>(&dst[q]) = v;
      if (!k4d_hit_in_feature(t, h)) { n_out++; continue; }
      if (n_out > 0) {
        if (n_copied < max_ml) *reinterpret_cast<uint4*>(&dst[n_copied]) = v;
        n_copied++;
      }
      n_pri++;
    }
  }
  const bool take = n_pri > 0 && n_pri <= max_ml;  // (m_bClampMaxMLmatches is -X: not combined with a table)
  need[i] = take ? 0 : 1;
  if (!take) return;
  // AlignRead's classification of eHRhits with LowHitInstances = n_pri and the wide call's LowMMCnt / NxtLowMMCnt (:9907-10023)
  k4_read_result r;
  r.hit_rslt = K4_HR_HITS; r.inst = n_pri; r.low_mm = w.low_mm; r.nxt_mm = w.nxt_mm;
  if (pe_mode >= 2) { r.nar = K4_NAR_ACCEPTED; r.num_hits = n_pri; }
  else if (!pe_mode || n_pri == 1) { r.nar = K4_NAR_ACCEPTED; r.num_hits = 1; }
  else { r.nar = K4_NAR_MULTIALIGN; r.num_hits = n_pri; }
  out_rr[i] = r;
  if (!sparse_hits)
    for (int q = n_pri; q < max_ml; q++) *reinterpret_cast<uint4*>(&out_hits[i * max_ml + q]) = make_uint4(0, 0, 0, 0);
}

// (c): where the listed reads lie
__global__ void __launch_bounds__(256) k4k_priority_gather(int64_t m, const uint32_t* __restrict__ idx, const uint64_t* __restrict__ offs,
                                                           const uint32_t* __restrict__ lens, uint64_t* __restrict__ offs2,
                                                           uint32_t* __restrict__ lens2) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const uint32_t i = idx[j];
  offs2[j] = offs[i];
  lens2[j] = lens[i];
}

// (d): record j of the normal call is read idx[j]'s
__global__ void __launch_bounds__(256) k4k_priority_scatter(int64_t m, int max_ml, const uint32_t* __restrict__ idx,
                                                            const k4_read_result* __restrict__ rr2, const k4_hit* __restrict__ hits2,
                                                            const k4_seg2* __restrict__ seg2_2, k4_read_result* __restrict__ out_rr,
                                                            k4_hit* __restrict__ out_hits, k4_seg2* __restrict__ out_seg2) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const int64_t i = idx[j];
  out_rr[i] = rr2[j];
  for (int q = 0; q < max_ml; q++)
    *reinterpret_cast<uint4*>(&out_hits[i * max_ml + q]) = *reinterpret_cast<const uint4*>(&hits2[j * max_ml + q]);
  if (out_seg2) *reinterpret_cast<uint4*>(&out_seg2[i]) = *reinterpret_cast<const uint4*>(&seg2_2[j]);
}

// FiltByPriorityRegions: an accepted read whose Seg[0] span (raw MatchLoci / MatchLen) is in no feature of its own sequence
__global__ void __launch_bounds__(256) k4k_filter_priority(K4PriTab t, K4ReadSet rs, k4_seg2* __restrict__ seg2,
                                                           unsigned long long* __restrict__ n_marked) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t n_reads = rs.n_reads;
  uint32_t marked = 0;
  for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); base < n_reads; base += stride) {
    const int64_t i = base + lane;
    bool drop = false;
    if (i < n_reads) {
      k4_hit h;
      if (rs.accepted(i, h)) drop = !k4d_hit_in_feature(t, h);
    }
    if (drop) {
      rs.reject(i, K4_NAR_REGIONFILT, false);  // NAR and NumHits; LowHitInstances stays (:4115-4116)
      rs.hit_ptr(i)->chrom_id = 0;             // both segments' ChromID (:4117-4118)
      if (seg2) seg2[i].chrom_id = 0;
    }
    marked += (uint32_t)__popcll(__ballot(drop));
  }
  if (lane == 0 && marked) atomicAdd(n_marked, (unsigned long long)marked);
}

struct NeedsNormal {
  const uint8_t* need;
  __device__ bool operator()(uint32_t i) const { return need[i] != 0; }
};

K4PriTab tab_of(const k4_index* ix) {
  K4PriTab t;
  t.off = ix->pri_off.as<uint32_t>();
  t.start = ix->pri_start.as<uint32_t>();
  t.end = ix->pri_end.as<uint32_t>();
  t.pt_off = ix->pri_pt_off.as<uint32_t>();
  t.pt = ix->pri_pt.as<uint32_t>();
  t.n_entries = ix->pri_n ? ix->d.n_entries : 0;  // (no table: no sequence has a feature, and the arrays are never read)
  return t;
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

// A view of one of the index's grow-only scratch blocks with the `alloc` the scaffold's helpers call: nothing is freed between
// calls (hipFree waits for the whole device, which would end the pipeline's overlap of copies and kernels).
struct GrowBuf {
  K4DevBuf* ext = nullptr;
  K4DevBuf own;
  void* p = nullptr;
  hipError_t alloc(size_t bytes) {
    K4DevBuf& t = ext ? *ext : own;
    const hipError_t e = t.reserve(bytes ? bytes : 1);
    p = t.p;
    return e;
  }
  template <typename T> T* as() const { return (T*)p; }
};

int launch_select(k4_index* ix, int64_t n, int max_ml, int pe_mode, int sparse_hits, const void* d_wide_rr, const void* d_wide_hits,
                  void* d_out_rr, void* d_out_hits, void* d_need, hipStream_t st) {
  hipLaunchKernelGGL(k4k_priority_select, dim3(blocks_for(n)), dim3(256), 0, st, tab_of(ix), n, max_ml, pe_mode, sparse_hits,
                     (const k4_read_result*)d_wide_rr, (const k4_hit*)d_wide_hits, (k4_read_result*)d_out_rr, (k4_hit*)d_out_hits, (uint8_t*)d_need);
  return k4_check_hip(ix, hipGetLastError(), "k4k_priority_select");
}

}  // namespace

extern "C" int k4_set_priority_regions(k4_index* ix, int64_t n_intervals, const uint32_t* entry_ids, const uint32_t* starts,
                                       const uint32_t* ends) {
  if (!ix || n_intervals < 0 || n_intervals >= 0x7FFFFFFFll) return K4_ERR_PARAMS;
  K4_HIP(ix, hipSetDevice(ix->device));
  K4_HIP(ix, hipDeviceSynchronize());  // (no call in flight reads the table that goes)
  ix->pri_n = 0;
  for (K4DevBuf* b : {&ix->pri_off, &ix->pri_start, &ix->pri_end, &ix->pri_pt_off, &ix->pri_pt}) b->release();
  if (n_intervals == 0) return K4_OK;
  if (!entry_ids || !starts || !ends) return k4_fail(ix, K4_ERR_PARAMS, "null buffer");
  const uint32_t n_ent = (uint32_t)ix->entries.size();
  struct Iv { uint32_t c, s, e; };
  std::vector<Iv> v, pts;
  for (int64_t k = 0; k < n_intervals; k++) {
    if (entry_ids[k] < 1 || entry_ids[k] > n_ent) return k4_fail(ix, K4_ERR_PARAMS, "priority region on sequence %u: no such sequence", entry_ids[k]);
    const Iv x = {entry_ids[k], starts[k], ends[k]};
    if (x.s >= 1 && x.e == x.s - 1) pts.push_back(x);  // a feature of no bases
    else if (x.s > x.e) return k4_fail(ix, K4_ERR_PARAMS, "priority region %u..%u: start behind end", x.s, x.e);
    else v.push_back(x);
  }
  const auto by_start = [](const Iv& a, const Iv& b) { return a.c != b.c ? a.c < b.c : a.s != b.s ? a.s < b.s : a.e < b.e; };
  std::sort(v.begin(), v.end(), by_start);
  std::sort(pts.begin(), pts.end(), by_start);
  // intervals that overlap or abut become one: "some feature meets [s, e]" is the same question of the union
  std::vector<uint32_t> off((size_t)n_ent + 2, 0), st, en, pt_off((size_t)n_ent + 2, 0), pt;
  for (const Iv& x : v) {
    const bool same = !st.empty() && off[x.c + 1] > 0;  // (off[c + 1] counts the intervals of c until the prefix sum below)
    if (same && (uint64_t)x.s <= (uint64_t)en.back() + 1) { en.back() = std::max(en.back(), x.e); continue; }
    st.push_back(x.s);
    en.push_back(x.e);
    off[x.c + 1]++;
  }
  for (const Iv& x : pts) { pt.push_back(x.s); pt_off[x.c + 1]++; }
  for (uint32_t c = 1; c <= n_ent; c++) { off[c + 1] += off[c]; pt_off[c + 1] += pt_off[c]; }  // off[c] = those of the sequences below c
  const std::pair<K4DevBuf*, const std::vector<uint32_t>*> up[5] = {{&ix->pri_off, &off}, {&ix->pri_start, &st}, {&ix->pri_end, &en},
                                                                    {&ix->pri_pt_off, &pt_off}, {&ix->pri_pt, &pt}};
  for (const auto& u : up) {
    K4_HIP(ix, u.first->alloc(u.second->size() * 4));
    if (!u.second->empty()) K4_HIP(ix, hipMemcpy(u.first->p, u.second->data(), u.second->size() * 4, hipMemcpyHostToDevice));
  }
  ix->pri_n = (uint32_t)(st.size() + pt.size());
  return K4_OK;
}

extern "C" int k4_priority_times(k4_index* ix, double ms3[3], uint64_t reads2[2]) {
  if (!ix || !ms3 || !reads2) return K4_ERR_PARAMS;
  for (int k = 0; k < 3; k++) { ms3[k] = ix->pri_ms[k]; ix->pri_ms[k] = 0; }
  for (int k = 0; k < 2; k++) { reads2[k] = ix->pri_reads[k]; ix->pri_reads[k] = 0; }
  return K4_OK;
}

extern "C" int k4_priority_select_dev(k4_index* ix, int64_t n_reads, int32_t max_ml, int32_t pe_mode, int32_t sparse_hits,
                                      const void* d_wide_rr, const void* d_wide_hits, void* d_out_rr, void* d_out_hits, void* d_need,
                                      void* stream) {
  if (!ix) return K4_ERR_PARAMS;
  if (max_ml < 1 || max_ml + K4_PRIORITY_EXACTS > 4096 || pe_mode < 0 || pe_mode > 2) return k4_fail(ix, K4_ERR_PARAMS, "kalign parameters out of range");
  if (n_reads < 0 || n_reads >= 0xFFFFFFF0ll) return k4_fail(ix, K4_ERR_PARAMS, "at most 2^32-16 reads per batch");
  if (n_reads == 0) return K4_OK;
  if (!d_wide_rr || !d_wide_hits || !d_out_rr || !d_out_hits || !d_need) return k4_fail(ix, K4_ERR_PARAMS, "null buffer");
  K4_HIP(ix, hipSetDevice(ix->device));
  return launch_select(ix, n_reads, max_ml, pe_mode, sparse_hits, d_wide_rr, d_wide_hits, d_out_rr, d_out_hits, d_need, (hipStream_t)stream);
}

int k4i_priority_kalign(k4_index* ix, const k4_kalign_params* p, int64_t n, int32_t max_len, const void* d_reads, const void* d_offs,
                        const void* d_lens, void* d_out, void* d_hits, void* d_seg2, void* stream, int sparse_hits) {
  if (!p) return K4_ERR_PARAMS;
  if (p->pe_mode >= 3) return k4_fail(ix, K4_ERR_UNSUPPORTED, "priority regions with -X / -N (pe_mode 3 / 4) are not built");
  if (p->max_ml < 1 || p->max_ml + K4_PRIORITY_EXACTS > 4096) return k4_fail(ix, K4_ERR_PARAMS, "kalign parameters out of range");
  if (n < 0 || (n > 0 && (!d_reads || !d_offs || !d_lens || !d_out || !d_hits))) return k4_fail(ix, K4_ERR_PARAMS, "null buffer");
  if (n == 0) return K4_OK;
  if (n >= 0xFFFFFFF0ll) return k4_fail(ix, K4_ERR_PARAMS, "at most 2^32-16 reads per batch");
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  const int max_ml = p->max_ml, wide_ml = max_ml + K4_PRIORITY_EXACTS;
  // the caller reserved for max_ml hits; the wide pass carries ten more (a workspace that is large enough is left as it is)
  K4_TRY(k4_reserve(ix, n, std::min<int32_t>(std::max<int32_t>(max_len, 1), K4_MAX_READ_LEN), wide_ml));
  const bool timed = ix->timing;
  auto tick = [&](std::chrono::steady_clock::time_point& t0, int slot) {
    if (!timed) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(st);
    const auto t1 = std::chrono::steady_clock::now();
    ix->pri_ms[slot] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return e;
  };
  std::chrono::steady_clock::time_point t0;
  if (timed) { K4_HIP(ix, hipStreamSynchronize(st)); t0 = std::chrono::steady_clock::now(); }
  // the scratch stays with the index and only grows: a call frees nothing
  K4DevBuf* const S = ix->pri_scratch;
  K4DevBuf &wide_rr = S[0], &wide_hits = S[1], &need = S[2], &offs2 = S[4], &lens2 = S[5], &rr2 = S[6], &hits2 = S[7], &seg2_2 = S[8];
  GrowBuf idx;
  idx.ext = &S[3];
  K4Scratch<GrowBuf> tmp;
  tmp.buf.ext = &S[9];
  // (a) MaxML + cPriorityExacts hits, microInDel 0, splice 0; everything else as given (:9702-9722)
  K4_HIP(ix, wide_rr.reserve((size_t)n * sizeof(k4_read_result)));
  K4_HIP(ix, wide_hits.reserve((size_t)n * wide_ml * sizeof(k4_hit)));
  K4_HIP(ix, need.reserve((size_t)n));
  k4_kalign_params wp = *p;
  wp.max_ml = wide_ml;
  wp.micro_indel_len = 0;
  wp.max_splice_junct_len = 0;
  K4_TRY(k4i_kalign_core(ix, &wp, n, max_len, d_reads, d_offs, d_lens, wide_rr.p, wide_hits.p, nullptr, stream, 1));
  K4_HIP(ix, tick(t0, 0));
  // (b)
  if (d_seg2) K4_HIP(ix, hipMemsetAsync(d_seg2, 0, (size_t)n * sizeof(k4_seg2), st));  // (a read the priority pass settles has one segment)
  K4_TRY(launch_select(ix, n, max_ml, (int)p->pe_mode, sparse_hits, wide_rr.p, wide_hits.p, d_out, d_hits, need.p, st));
  // the reads that need the normal call, listed (the scaffold's k4s_select_indices, with the temporary kept as well)
  const size_t list = ((size_t)n * 4 + 7) & ~(size_t)7;
  K4_HIP(ix, idx.alloc(list + 8));
  uint64_t* d_m = reinterpret_cast<uint64_t*>(idx.as<char>() + list);
  const NeedsNormal pred{need.as<uint8_t>()};
  K4_TRY(k4s_two_calls<GrowBuf>(ix, "rocprim::select", [&](void* t, size_t& tb) {
    return rocprim::select(t, tb, rocprim::counting_iterator<uint32_t>(0), idx.as<uint32_t>(), d_m, (size_t)n, pred, st);
  }, &tmp));
  uint64_t m = 0;
  K4_TRY(k4s_read_back(ix, &m, d_m, st));
  K4_HIP(ix, tick(t0, 1));
  ix->pri_reads[0] += (uint64_t)n;
  ix->pri_reads[1] += m;
  if (m == 0) return K4_OK;
  // (c) the normal call (:9799-9816) over the reads that need it, from fresh counters (:9766-9768)
  K4_HIP(ix, offs2.reserve((size_t)m * 8));
  K4_HIP(ix, lens2.reserve((size_t)m * 4));
  K4_HIP(ix, rr2.reserve((size_t)m * sizeof(k4_read_result)));
  K4_HIP(ix, hits2.reserve((size_t)m * max_ml * sizeof(k4_hit)));
  if (d_seg2) K4_HIP(ix, seg2_2.reserve((size_t)m * sizeof(k4_seg2)));
  hipLaunchKernelGGL(k4k_priority_gather, dim3(blocks_for((int64_t)m)), dim3(256), 0, st, (int64_t)m, idx.as<uint32_t>(), (const uint64_t*)d_offs,
                     (const uint32_t*)d_lens, offs2.as<uint64_t>(), lens2.as<uint32_t>());
  K4_HIP(ix, hipGetLastError());
  K4_TRY(k4i_kalign_core(ix, p, (int64_t)m, max_len, d_reads, offs2.p, lens2.p, rr2.p, hits2.p, d_seg2 ? seg2_2.p : nullptr, stream, 0));
  // (d)
  hipLaunchKernelGGL(k4k_priority_scatter, dim3(blocks_for((int64_t)m)), dim3(256), 0, st, (int64_t)m, max_ml, idx.as<uint32_t>(),
                     rr2.as<k4_read_result>(), hits2.as<k4_hit>(), d_seg2 ? seg2_2.as<k4_seg2>() : nullptr, (k4_read_result*)d_out, (k4_hit*)d_hits,
                     (k4_seg2*)d_seg2);
  K4_HIP(ix, hipGetLastError());
  K4_HIP(ix, tick(t0, 2));
  return K4_OK;
}

extern "C" int k4_filter_priority_regions_dev(k4_index* ix, int pe, int64_t n_reads, int32_t max_ml, void* d_rr_or_pe, void* d_hits,
                                              void* d_seg2, int64_t* n_removed, void* stream) {
  if (!ix) return K4_ERR_PARAMS;
  if (n_removed) *n_removed = 0;
  if (n_reads <= 0) return K4_OK;
  K4ReadSet rs;
  K4_TRY(k4s_read_set(ix, pe, n_reads, d_rr_or_pe, d_hits, max_ml, d_rr_or_pe, nullptr, nullptr, nullptr, nullptr, K4RS_HITS, &rs));
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  K4DevBuf cnt;
  K4_HIP(ix, cnt.alloc(8));
  K4_HIP(ix, hipMemsetAsync(cnt.p, 0, 8, st));
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix->device) != hipSuccess || cus <= 0) cus = 256;
  const int64_t blocks = std::min<int64_t>((n_reads + 255) / 256, (int64_t)cus * 8);
  hipLaunchKernelGGL(k4k_filter_priority, dim3((unsigned)blocks), dim3(256), 0, st, tab_of(ix), rs, pe ? nullptr : (k4_seg2*)d_seg2,
                     cnt.as<unsigned long long>());
  K4_HIP(ix, hipGetLastError());
  unsigned long long c = 0;
  K4_TRY(k4s_read_back(ix, &c, cnt.p, st));
  if (n_removed) *n_removed = (int64_t)c;
  ix->filter_prior[K4_NAR_ACCEPTED] += c;
  return K4_OK;
}
